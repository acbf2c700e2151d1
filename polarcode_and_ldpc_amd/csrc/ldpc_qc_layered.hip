// Layered normalised min-sum for quasi-cyclic LDPC codes on gfx950 (MI355X).
// H is mb x nb blocks of Z x Z, each zero or an identity shifted cyclically by
// s: H[i Z + r, j Z + (r + s) % Z] = 1.  Build-defined, as ldpc_layered.hip,
// and by definition equal to that decoder on the expanded H with the block rows
// as layers: the check state, its packing and the rule are ldpc_lms_check.hpp's
// text, the position of an input in its check is the rank of its block column
// among the row's non-zero blocks (its CSR position).
//
// What the structure buys over ldpc_layered_kernel:
//   - no row_ptr / col_idx / layer_rows: a layer is (block row, degree d, d
//     (block column, shift) pairs), the same for every lane, read from a stream
//     at wave-uniform addresses (scalar loads), and the variable of check r is
//     col Z + (r + s >= Z ? r + s - Z : r + s): consecutive lanes, consecutive P;
//   - every check of a layer has the layer's degree: no divergence in the loops;
//   - DCAP > 0: for d <= DCAP the q_j of the first pass stay in registers for
//     the second, one gather per edge.  DCAP == 0: the two-pass form of
//     lms_check_update (degrees up to 2047).
// Mapping: one thread per check of the current block row.
//   SUBWAVE (Z <= 64): fpw = 64 / Z frames share a wavefront, lane l = frame
//     l / Z, check l % Z; several wavefronts per workgroup; layers ordered by the
//     wavefront-level fence only, no workgroup barrier anywhere.  Each frame of
//     a wavefront stops on its own zero syndrome (its lanes stop updating); the
//     wavefront runs until all its frames have stopped.
//   block (Z > 64): one frame per workgroup of roundup64(Z) threads, one
//     __syncthreads per layer, the early-stop vote as lms_wg_any.
// State per frame as ldpc_layered.hip (P[n], double2 minima and mw meta words
// per check), in LDS or (GLOBAL) in the frame's slice of the workspace.
// Single precision (PL_LDPC_QC_F32): the same text instantiated with T = float
// -- P[n] float, float2 minima, the same meta words -- every operation one IEEE
// binary32 operation (no FMA contraction: -ffp-contract=off; no double in the
// arithmetic; subnormals kept: the default denormal mode), so the results equal
// a NumPy float32 restatement bit for bit.  The T = double instances are the
// code they were before T existed.
#include "common.hpp"
#include "internal.hpp"
#include "ldpc_lms_check.hpp"

namespace pl {

// the variable check r of a block row reads through the block (col, s)
PL_DEV int qc_var(int col, int s, int r, int z) {
    const int t = r + s;
    return col * z + (t >= z ? t - z : t);
}

// One layered update of check r of a block row of degree d >= 2; pr: its d
// (block column, shift) pairs.  DCAP > 0 requires d <= DCAP <= 32, so the
// negative flags of a check are one word.  norm: the normalisation in the state
// type (the kernel converts it once, at entry).
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
template <typename T, typename IO, int DCAP, bool SUBWAVE, bool GLOBAL>
__global__ void __launch_bounds__(SUBWAVE ? 256 : 1024)
ldpc_qc_kernel(QcGeom g, const int32_t* __restrict__ tab, const IO* __restrict__ llr, int64_t ld,
               uint8_t* __restrict__ bits, int32_t* __restrict__ iters, IO* __restrict__ post, int64_t ld_post,
               int64_t batch, unsigned char* __restrict__ work) {
    using Pair = typename LmsNum<T>::Pair;
    // a single-precision plan's g.norm already holds a float's value (qc_plan_build rounds it once), so this
    // one conversion is exact and no double is left in the float instances' iteration loop
    const T norm = (T)g.norm;
    extern __shared__ __align__(16) unsigned char qc_smem[];
    const int z = g.z;
    int r, f = 0, slot = 0;
    int64_t frame;
    bool mine;  // this lane holds check r of a frame of the batch
    if (SUBWAVE) {
        const int wv = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
        const int64_t wave0 = ((int64_t)blockIdx.x * g.fpb + wv) * g.fpw;
        if (wave0 >= batch) return;  // a ragged last workgroup (no workgroup barrier below)
        f = lane / z;
        r = lane - f * z;
        frame = wave0 + f;
        mine = f < g.fpw && frame < batch;  // idle lanes and frames past the batch: masked from the start
        slot = mine ? wv * g.fpw + f : 0;
        if (!mine) frame = 0;
    } else {
        r = (int)threadIdx.x;
        frame = (int64_t)blockIdx.x;
        mine = r < z;
    }
    unsigned char* const base = GLOBAL ? work + (size_t)frame * (size_t)g.state_bytes
                                       : qc_smem + (size_t)slot * (size_t)g.state_bytes;
    T* const P = reinterpret_cast<T*>(base);
    Pair* const MM = reinterpret_cast<Pair*>(base + g.off_mm);
    uint32_t* const META = reinterpret_cast<uint32_t*>(base + g.off_meta);
    uint32_t* const vote = reinterpret_cast<uint32_t*>(qc_smem + (GLOBAL ? 0 : g.state_bytes));  // block mapping: [2][16]
    const IO* const lf = llr + frame * ld;
    // the lanes that move a frame's P in and out: its Z lanes, or the whole workgroup
    const bool io = SUBWAVE ? mine : true;
    const int v0 = SUBWAVE ? r : (int)threadIdx.x, vstep = SUBWAVE ? z : (int)blockDim.x;

    if (io)
        for (int v = v0; v < g.n; v += vstep) P[v] = (T)lf[v];
    lms_sync<SUBWAVE>();

    bool live = mine;  // SUBWAVE: cleared when the lane's frame has stopped
    int done = g.max_iter;
    for (int it = 0; it < g.max_iter; ++it) {
        const int32_t* t = tab;
        for (int l = 0; l < g.mb; ++l) {
            const int i = t[0], d = t[1];
            if (d > 0) {  // the same in every lane
                if (live) {
                    const int c = i * z + r;
                    qc_check_update<T, DCAP>(g, t + 2, d, r, P, MM + c, META + (size_t)c * g.mw, it == 0, norm);
                }
                lms_sync<SUBWAVE>();
            }
            t += 2 + 2 * d;
        }
        if (g.early_stop) {
            bool bad = false;
            if (live) {
                t = tab;
                for (int l = 0; l < g.mb; ++l) {
                    const int d = t[1];
                    uint32_t par = 0;
                    for (int j = 0; j < d; ++j) par ^= P[qc_var(t[2 + 2 * j], t[3 + 2 * j], r, z)] <= T(0) ? 1u : 0u;
                    bad |= par != 0u;
                    t += 2 + 2 * d;
                }
            }
            if (SUBWAVE) {
                const unsigned long long badm = __ballot(bad);
                lms_sync<true>();  // the next iteration's stores to P stay behind these loads
                if (live) {
                    const unsigned long long fm = (z == 64 ? ~0ull : ((1ull << z) - 1ull)) << (f * z);
                    if ((badm & fm) == 0ull) { done = it + 1; live = false; }
                }
                if (__ballot(live) == 0ull) break;
            } else {
                if (!lms_wg_any(bad, vote, it & 1)) { done = it + 1; break; }
            }
        }
    }

    if (io) {
        uint8_t* const bf = bits + frame * (int64_t)g.n;
        for (int v = v0; v < g.n; v += vstep) {
            const T x = P[v];
            bf[v] = x <= T(0) ? 1 : 0;
            if (post) post[frame * ld_post + v] = (IO)x;
        }
    }
    if (iters && mine && r == 0) iters[frame] = done;
}

template <typename T, typename IO, int DCAP>
static void* qc_pick_at(const QcGeom& g) {
    if (g.subwave)
        return g.use_global ? (void*)ldpc_qc_kernel<T, IO, DCAP, true, true>
                            : (void*)ldpc_qc_kernel<T, IO, DCAP, true, false>;
    return g.use_global ? (void*)ldpc_qc_kernel<T, IO, DCAP, false, true>
                        : (void*)ldpc_qc_kernel<T, IO, DCAP, false, false>;
}
template <typename T, typename IO>
static void* qc_pick_t(const QcGeom& g) {
    switch (g.dcap) {
        case 8: return qc_pick_at<T, IO, 8>(g);
        case 16: return qc_pick_at<T, IO, 16>(g);
        case 32: return qc_pick_at<T, IO, 32>(g);
        default: return qc_pick_at<T, IO, 0>(g);
    }
}
// the instance of a plan for llr / post of type IO (a float plan takes both, an fp64 plan double only)
template <typename IO>
static void* qc_pick(const QcGeom& g, bool f32) {
    if (f32) return qc_pick_t<float, IO>(g);
    if constexpr (sizeof(IO) == sizeof(double)) return qc_pick_t<double, double>(g);
    return nullptr;
}

hipError_t qc_prepare(const QcGeom& g, bool f32) {
    const hipError_t e =
        hipFuncSetAttribute(qc_pick<double>(g, f32), hipFuncAttributeMaxDynamicSharedMemorySize, g.lds_bytes);
    if (e != hipSuccess || !f32) return e;
    return hipFuncSetAttribute(qc_pick<float>(g, true), hipFuncAttributeMaxDynamicSharedMemorySize, g.lds_bytes);
}

template <typename IO>
static hipError_t qc_launch_io(const QcGeom& g, bool f32, const int32_t* tab, const IO* llr, int64_t ld, uint8_t* bits,
                               int32_t* iters, IO* post, int64_t ld_post, int64_t batch, unsigned char* work,
                               hipStream_t s) {
    void* const fn = qc_pick<IO>(g, f32);
    if (!fn) return hipErrorInvalidValue;  // float llr on an fp64 plan: capi.cpp refuses it first
    QcGeom gg = g;
    const int64_t fpg = (int64_t)g.fpw * g.fpb;  // frames per workgroup
    void* args[] = {&gg, (void*)&tab, (void*)&llr, (void*)&ld, (void*)&bits, (void*)&iters, (void*)&post,
                    (void*)&ld_post, (void*)&batch, (void*)&work};
    return hipLaunchKernel(fn, dim3((unsigned)((batch + fpg - 1) / fpg)), dim3(g.threads), args, g.lds_bytes, s);
}
hipError_t qc_launch(const QcGeom& g, bool f32, const int32_t* tab, const double* llr, int64_t ld, uint8_t* bits,
                     int32_t* iters, double* post, int64_t ld_post, int64_t batch, unsigned char* work, hipStream_t s) {
    return qc_launch_io(g, f32, tab, llr, ld, bits, iters, post, ld_post, batch, work, s);
}
hipError_t qc_launch(const QcGeom& g, const int32_t* tab, const float* llr, int64_t ld, uint8_t* bits, int32_t* iters,
                     float* post, int64_t ld_post, int64_t batch, unsigned char* work, hipStream_t s) {
    return qc_launch_io(g, true, tab, llr, ld, bits, iters, post, ld_post, batch, work, s);
}

}  // namespace pl

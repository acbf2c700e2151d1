// Layered (row-serial) normalised min-sum LDPC decoder with posterior output
// for gfx950 (MI355X).  Build-defined extension: the reference has flooding
// decoders only; the check rule is MSDecoder._check_node_update_ms
// (src/ldpc/decoder.py:257-287) applied layer by layer to the posteriors.
//
//   P[v] = llr[v], R = 0
//   per iteration, per layer (in the given order), per check c of the layer:
//     q_j = P[v_j] - R_cj;  R_cj = (prod_{k != j} sign(q_k) * min_{k != j} |q_k|) * norm;
//     P[v_j] = q_j + R_cj
//   decisions P <= 0; early stop when every check is satisfied.
// A layer's checks share no variable (the plan checks it), so they run in
// parallel; layers are separated by a barrier.
//
// Mapping: one thread per check of the current layer.
//   WAVE  (largest layer <= 64 checks): one wavefront per frame, several frames
//         per workgroup; layers are ordered by a wavefront-level fence only, no
//         workgroup barrier anywhere, so a wavefront past the batch just leaves.
//   block (otherwise): one workgroup per frame, one __syncthreads per layer.
// State per frame: P[n] fp64 and, per check, a compressed min-sum state in the
// manner of ldpc.hip's ldpc_ms_compact_kernel: the two smallest |q| (NaNs left
// out), the position of the smallest, NaN / zero counts, the position of the
// first NaN, the parity of negatives and one negative flag per position.
// Unlike that kernel's pre-scaled variant the magnitudes are stored NOT
// multiplied by the normalization: lms_c2v rebuilds R_cj per edge as
// (sign product * min) * norm, ms_check's order of operations, which is exact
// for every normalization (|norm| > 1, negative, 0, non-finite), where a
// pre-scaled min could overflow or lose a NaN.  Posteriors therefore equal the
// NumPy definition bit for bit.  Row degrees up to 2047 (11-bit positions).
// The state lives in LDS, or (GLOBAL) in a per-frame slice of the workspace.
// The check state and its helpers are in ldpc_lms_check.hpp (shared with
// ldpc_qc_layered.hip).
#include "common.hpp"
#include "internal.hpp"
#include "ldpc_lms_check.hpp"

namespace pl {

// One layered update of check c (degree d >= 2).  Two passes over its inputs:
// the first forms q_j and the new state, the second forms q_j again (P and the
// old state are untouched until then: no other check of the layer shares a
// variable) and writes P[v_j] = q_j + R_cj.
PL_DEV void lms_check_update(const LmsGeom& g, const int32_t* __restrict__ col, int d, double* P, double2* mmp,
                             uint32_t* mw, bool first) {
    const bool small = g.mw == 1;
    LmsCheck old{};
    uint32_t w0 = 0;
    if (!first) {
        const double2 mm = *mmp;
        old.min1 = mm.x; old.min2 = mm.y;
        w0 = mw[0];
        lms_unpack(w0, small, old);
    }
    LmsCheck nw{};
    nw.min1 = __builtin_inf(); nw.min2 = __builtin_inf();
    uint32_t negw = small ? (w0 >> 16) : 0u;
    for (int j = 0; j < d; ++j) {
        if (!small && !first && (j & 31) == 0) negw = mw[1 + (j >> 5)];
        const double p = P[col[j]];
        const double r = first ? 0.0 : lms_c2v(old, (negw >> (j & 31)) & 1u, (uint32_t)j, g.norm);
        const double q = p - r;
        if (__builtin_isnan(q)) {
            if (nw.ncnt == 0u) nw.nidx = (uint32_t)j;
            nw.ncnt = nw.ncnt < 2u ? nw.ncnt + 1u : 2u;
        } else {
            const double a = fabs(q);
            if (a < nw.min1) { nw.min2 = nw.min1; nw.min1 = a; nw.idx1 = (uint32_t)j; }
            else if (a < nw.min2) nw.min2 = a;
        }
        if (q == 0.0) nw.zcnt = nw.zcnt < 2u ? nw.zcnt + 1u : 2u;
        if (q < 0.0) nw.par ^= 1u;
    }
    uint32_t acc = 0;
    negw = small ? (w0 >> 16) : 0u;
    for (int j = 0; j < d; ++j) {
        if (!small && !first && (j & 31) == 0) negw = mw[1 + (j >> 5)];
        const int v = col[j];
        const double p = P[v];
        const double r = first ? 0.0 : lms_c2v(old, (negw >> (j & 31)) & 1u, (uint32_t)j, g.norm);
        const double q = p - r;
        const uint32_t nb = q < 0.0 ? 1u : 0u;
        P[v] = q + lms_c2v(nw, nb, (uint32_t)j, g.norm);
        acc |= nb << (j & 31);
        if (!small && ((j & 31) == 31 || j == d - 1)) { mw[1 + (j >> 5)] = acc; acc = 0; }
    }
    *mmp = make_double2(nw.min1, nw.min2);
    mw[0] = lms_pack(nw, small, acc);
}

template <bool WAVE, bool GLOBAL>
__global__ void __launch_bounds__(1024)
ldpc_layered_kernel(LmsGeom g, LmsDev dv, const double* __restrict__ llr, int64_t ld, uint8_t* __restrict__ bits,
                    int32_t* __restrict__ iters, double* __restrict__ post, int64_t ld_post, int64_t batch,
                    unsigned char* __restrict__ work) {
    extern __shared__ __align__(16) unsigned char lms_smem[];
    const int wv = (int)(threadIdx.x >> 6);
    const int lane = WAVE ? (int)(threadIdx.x & 63u) : (int)threadIdx.x;
    const int nthr = WAVE ? 64 : (int)blockDim.x;
    const int64_t frame = WAVE ? (int64_t)blockIdx.x * g.fpb + wv : (int64_t)blockIdx.x;
    if (frame >= batch) return;  // WAVE: a ragged last workgroup (no workgroup barrier below); block: never
    unsigned char* const base = GLOBAL ? work + (size_t)frame * (size_t)g.state_bytes
                                       : lms_smem + (WAVE ? (size_t)wv * (size_t)g.state_bytes : (size_t)0);
    double* const P = reinterpret_cast<double*>(base);
    double2* const MM = reinterpret_cast<double2*>(base + g.off_mm);
    uint32_t* const META = reinterpret_cast<uint32_t*>(base + g.off_meta);
    uint32_t* const vote = reinterpret_cast<uint32_t*>(lms_smem + (GLOBAL ? 0 : g.state_bytes));  // block mapping: [2][16]
    const double* const lf = llr + frame * ld;

    for (int v = lane; v < g.n; v += nthr) P[v] = lf[v];
    lms_sync<WAVE>();

    int done = g.max_iter;
    for (int it = 0; it < g.max_iter; ++it) {
        for (int l = 0; l < g.n_layers; ++l) {
            const int k1 = dv.layer_ptr[l + 1];
            for (int k = dv.layer_ptr[l] + lane; k < k1; k += nthr) {
                const int c = dv.layer_rows[k];
                const int e0 = dv.row_ptr[c], d = dv.row_ptr[c + 1] - e0;
                if (d > 0) lms_check_update(g, dv.col_idx + e0, d, P, MM + c, META + (size_t)c * g.mw, it == 0);
            }
            lms_sync<WAVE>();
        }
        if (g.early_stop) {
            bool bad = false;
            for (int c = lane; c < g.m; c += nthr) {
                uint32_t par = 0;
                for (int e = dv.row_ptr[c]; e < dv.row_ptr[c + 1]; ++e) par ^= P[dv.col_idx[e]] <= 0.0 ? 1u : 0u;
                bad |= par != 0u;
            }
            bool any;
            if (WAVE) {
                any = __ballot(bad) != 0;
                lms_sync<true>();  // the next iteration's stores to P stay behind these loads
            } else {
                any = lms_wg_any(bad, vote, it & 1);
            }
            if (!any) { done = it + 1; break; }
        }
    }

    uint8_t* const bf = bits + frame * (int64_t)g.n;
    for (int v = lane; v < g.n; v += nthr) {
        const double t = P[v];
        bf[v] = t <= 0.0 ? 1 : 0;
        if (post) post[frame * ld_post + v] = t;
    }
    if (iters && lane == 0) iters[frame] = done;
}

static void* lms_pick(const LmsGeom& g) {
    if (g.wave) return g.use_global ? (void*)ldpc_layered_kernel<true, true> : (void*)ldpc_layered_kernel<true, false>;
    return g.use_global ? (void*)ldpc_layered_kernel<false, true> : (void*)ldpc_layered_kernel<false, false>;
}

hipError_t lms_prepare(const LmsGeom& g) {
    return hipFuncSetAttribute(lms_pick(g), hipFuncAttributeMaxDynamicSharedMemorySize, g.lds_bytes);
}

hipError_t lms_launch(const LmsGeom& g, const LmsDev& d, const double* llr, int64_t ld, uint8_t* bits, int32_t* iters,
                      double* post, int64_t ld_post, int64_t batch, unsigned char* work, hipStream_t s) {
    LmsGeom gg = g;
    LmsDev dd = d;
    void* args[] = {&gg, &dd, (void*)&llr, (void*)&ld, (void*)&bits, (void*)&iters, (void*)&post, (void*)&ld_post,
                    (void*)&batch, (void*)&work};
    return hipLaunchKernel(lms_pick(g), dim3((unsigned)((batch + g.fpb - 1) / g.fpb)), dim3(g.threads), args,
                           g.lds_bytes, s);
}

}  // namespace pl

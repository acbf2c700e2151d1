// The frame skeleton of the quasi-cyclic layered decoders on gfx950 (MI355X):
// everything ldpc_qc_layered.hip (min-sum, fp64 and fp32), ldpc_qc_fixed.hip
// (min-sum, int8) and ldpc_qc_bp.hip (sum-product, fp64) do alike -- lanes to (frame, check), the state's home, the load of P,
// the walk over the layer stream, the syndrome pass, the stop votes, the hard
// decision and the stores -- and the choice and launch of an instance.  Device
// code; each .hip instantiates its own kernels from it.
//
// H is mb x nb blocks of Z x Z, each zero or an identity shifted cyclically by
// s; a block row is a layer.  A layer of the stream is (block row, degree d, d
// (block column, shift) pairs), the same for every lane, read at wave-uniform
// addresses (scalar loads); every check of a layer has the layer's degree, so
// the loops do not diverge.
// Mapping: one thread per check of the current block row.
//   SUBWAVE (Z <= 64): fpw = 64 / Z frames share a wavefront, lane l = frame
//     l / Z, check l % Z; several wavefronts per workgroup; layers ordered by the
//     wavefront-level fence only, no workgroup barrier anywhere.  Each frame of
//     a wavefront stops on its own zero syndrome (its lanes stop updating); the
//     wavefront runs until all its frames have stopped.
//   block (Z > 64): one frame per workgroup of roundup64(Z) threads, one
//     __syncthreads per layer, the early-stop vote as lms_wg_any.
// DCAP > 0: for d <= DCAP the q_j of a check's first pass stay in registers for
// the second, one gather per edge.  DCAP == 0: the two-pass form (degrees up to
// 2047).
// State per frame: state_bytes in LDS or (GLOBAL) in the frame's slice of the
// workspace, laid out by the rule.
//
// A Rule is what the arithmetics do not share:
//   Geom, IO, Elem   the kernel's geometry argument (a QcMap and the rule's own
//                    fields), the type of llr and post, the type of P
//   Rule(g, base)    carves a frame's state out of its state_bytes at base; P is a member
//   load(g, x)       the state element of the LLR x
//   update<DCAP>(g, pr, d, r, c, first)
//                    one layered update of check c = (block row) Z + r of degree d >= 2,
//                    pr its d (block column, shift) pairs; first: the check's state holds
//                    nothing yet
//   A rule that declares kEdgeOffset = true takes one more argument behind first: the number of
//                    blocks in the earlier layers of the stream (where a per-edge state of the layer begins)
// In all of them a bit is 1 and a parity term is set where P[v] <= 0, and post is (IO)P[v].
#pragma once
#include <type_traits>

#include "common.hpp"
#include "internal.hpp"
#include "ldpc_lms_check.hpp"  // lms_sync, lms_wg_any

namespace pl {

// the variable check r of a block row reads through the block (col, s)
PL_DEV int qc_var(int col, int s, int r, int z) {
    const int t = r + s;
    return col * z + (t >= z ? t - z : t);
}

// whether a rule asks for the layer's edge offset (Rule::kEdgeOffset)
template <class Rule, class = void>
struct QcRuleEdgeOffset { static constexpr bool value = false; };
template <class Rule>
struct QcRuleEdgeOffset<Rule, std::void_t<decltype(Rule::kEdgeOffset)>> {
    static constexpr bool value = Rule::kEdgeOffset;
};
// the stream walk's count of the blocks behind it: an int for the rules that ask, nothing for the others
struct QcNoEdgeOffset {
    PL_DEV void operator+=(int) {}
};

template <class Rule, int DCAP, bool SUBWAVE, bool GLOBAL>
__global__ void __launch_bounds__(SUBWAVE ? 256 : 1024)
qc_frame_kernel(typename Rule::Geom g, const int32_t* __restrict__ tab, const typename Rule::IO* __restrict__ llr,
                int64_t ld, uint8_t* __restrict__ bits, int32_t* __restrict__ iters,
                typename Rule::IO* __restrict__ post, int64_t ld_post, int64_t batch,
                unsigned char* __restrict__ work) {
    using IO = typename Rule::IO;
    using Elem = typename Rule::Elem;
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
    const Rule rule(g, base);
    Elem* const P = rule.P;
    uint32_t* const vote = reinterpret_cast<uint32_t*>(qc_smem + (GLOBAL ? 0 : g.state_bytes));  // block mapping: [2][16]
    const IO* const lf = llr + frame * ld;
    // the lanes that move a frame's P in and out: its Z lanes, or the whole workgroup
    const bool io = SUBWAVE ? mine : true;
    const int v0 = SUBWAVE ? r : (int)threadIdx.x, vstep = SUBWAVE ? z : (int)blockDim.x;

    if (io)
        for (int v = v0; v < g.n; v += vstep) P[v] = Rule::load(g, lf[v]);
    lms_sync<SUBWAVE>();

    bool live = mine;  // SUBWAVE: cleared when the lane's frame has stopped
    int done = g.max_iter;
    for (int it = 0; it < g.max_iter; ++it) {
        const int32_t* t = tab;
        std::conditional_t<QcRuleEdgeOffset<Rule>::value, int, QcNoEdgeOffset> e0{};  // blocks of the layers walked
        for (int l = 0; l < g.mb; ++l) {
            const int i = t[0], d = t[1];
            if (d > 0) {  // the same in every lane
                if constexpr (QcRuleEdgeOffset<Rule>::value) {
                    if (live) rule.template update<DCAP>(g, t + 2, d, r, i * z + r, it == 0, e0);
                } else {
                    if (live) rule.template update<DCAP>(g, t + 2, d, r, i * z + r, it == 0);
                }
                lms_sync<SUBWAVE>();
            }
            e0 += d;
            t += 2 + 2 * d;
        }
        if (g.early_stop) {
            bool bad = false;
            if (live) {
                t = tab;
                for (int l = 0; l < g.mb; ++l) {
                    const int d = t[1];
                    uint32_t par = 0;
                    for (int j = 0; j < d; ++j) par ^= P[qc_var(t[2 + 2 * j], t[3 + 2 * j], r, z)] <= Elem(0) ? 1u : 0u;
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
            const Elem x = P[v];
            bf[v] = x <= Elem(0) ? 1 : 0;
            if (post) post[frame * ld_post + v] = (IO)x;
        }
    }
    if (iters && mine && r == 0) iters[frame] = done;
}

// ---- the instance of a plan, and its launch ----
template <class Rule, int DCAP>
static void* qc_frame_pick_at(const QcMap& g) {
    if (g.subwave)
        return g.use_global ? (void*)qc_frame_kernel<Rule, DCAP, true, true>
                            : (void*)qc_frame_kernel<Rule, DCAP, true, false>;
    return g.use_global ? (void*)qc_frame_kernel<Rule, DCAP, false, true>
                        : (void*)qc_frame_kernel<Rule, DCAP, false, false>;
}
template <class Rule>
static void* qc_frame_pick(const QcMap& g) {
    switch (g.dcap) {
        case 8: return qc_frame_pick_at<Rule, 8>(g);
        case 16: return qc_frame_pick_at<Rule, 16>(g);
        case 32: return qc_frame_pick_at<Rule, 32>(g);
        default: return qc_frame_pick_at<Rule, 0>(g);
    }
}

template <class Rule>
static hipError_t qc_frame_prepare(const QcMap& g) {
    return hipFuncSetAttribute(qc_frame_pick<Rule>(g), hipFuncAttributeMaxDynamicSharedMemorySize, g.lds_bytes);
}

template <class Rule>
static hipError_t qc_frame_launch(const typename Rule::Geom& g, const int32_t* tab, const typename Rule::IO* llr,
                                  int64_t ld, uint8_t* bits, int32_t* iters, typename Rule::IO* post, int64_t ld_post,
                                  int64_t batch, unsigned char* work, hipStream_t s) {
    typename Rule::Geom gg = g;
    const int64_t fpg = (int64_t)g.fpw * g.fpb;  // frames per workgroup
    void* args[] = {&gg, (void*)&tab, (void*)&llr, (void*)&ld, (void*)&bits, (void*)&iters, (void*)&post,
                    (void*)&ld_post, (void*)&batch, (void*)&work};
    return hipLaunchKernel(qc_frame_pick<Rule>(g), dim3((unsigned)((batch + fpg - 1) / fpg)), dim3(g.threads), args,
                           g.lds_bytes, s);
}

}  // namespace pl

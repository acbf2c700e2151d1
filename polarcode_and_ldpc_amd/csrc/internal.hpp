// Host-side internal interface between the C-ABI (capi.cpp) and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "interleave_check.hpp"
#include "ldpc_plan.hpp"

#ifndef PL_METRIC_FUSED_NMAX
// polar tree instances with n <= this use the fused log1p(exp(-x))
// (log1p_exp_neg): N=1024 L=8 -1.9 %, L=32 -2.6 % (round 4); N=4096 L=8 +3.6 %
// then (register allocation), -0.6 % with round 5's 16 waves per CU and
// de-duplicated fused top -- every tree instance (n <= 12) now uses it
#define PL_METRIC_FUSED_NMAX 12
#endif

namespace pl {

constexpr int kMaxDepth = 15;  // N <= 2^15

// What pl_plan_get_info reports about a polar plan's kernel.
struct PolarGeom {
    int N, K, F;
    int lds_bytes;
};

// Lane-per-path decoder (polar_lane.hip): one lane = one list path, 64/lcap
// frames per wavefront; tree depths tiered over registers / LDS / workspace.
struct LaneGeom {
    int N, n, K, Lsz, lcap, F, B, D, Dl, cw;
    int lw;                        // lanes per workgroup: 64, or lcap (> 64: one frame per workgroup)
    int lds_bytes, lds_final;
    int lds_xchg;                  // lcap > 64: metric / row / rank exchange scratch [lw]
    int lds_pool[kMaxDepth + 2];   // byte offset of LDS pool depth d (Dl <= d <= D): [2^(n-d)][lw] f64
    int lds_bl[kMaxDepth + 2];     // byte offset of single-word beta depth d: [lw] u32
    int bl_words[kMaxDepth + 2];   // beta words per slot at depth d
    int64_t ws_pool[kMaxDepth + 2];  // workspace byte offset of pool depth d (F <= d < Dl)
    int64_t ws_bl[kMaxDepth + 2];    // workspace byte offset of multi-word beta depth d: [words][lw] u32
    int64_t ws_walk;                 // [2][cw][lw] u32 walk buffers
    int64_t ws_bytes;                // workspace bytes per workgroup
};
int lane_geom(int N, int K, int list_size, int F, int lds_budget, LaneGeom* g);
hipError_t lane_prepare(const LaneGeom& g, bool sc, int* max_blocks_per_cu);
hipError_t lane_launch(const LaneGeom& g, bool sc, const double* llr, int64_t ld, uint8_t* out,
                       const uint32_t* frozen_dec, const int32_t* info_pos, int64_t batch, unsigned char* ws,
                       int grid, const uint32_t* crc_g, uint64_t* nan_masks, hipStream_t s);

// v4 lane-per-path decoder with compile-time geometry (polar_tree.hip); built
// for the (n, list capacity) pairs in its table, polar_lane.hip covers the rest.
struct TreeInfo {
    void* fn;
    void* fn_stamps;
    void* fn_ds[2];  // PL_DIAG: dead-store record / replay instances (headline geometry only)
    int lds_bytes;
    int64_t ws_bytes;  // workspace bytes per resident wavefront
    int F, DL, fpw;
};
bool tree_lookup(int n, int lcap, bool sc, TreeInfo* info);
// a list instance for batches that fit the device at its 8 waves per CU (one
// more LDS depth, 2-wave register budget), if (n, lcap) has one
bool tree_lookup_small(int n, int lcap, bool sc, TreeInfo* info);
// The tree and lane kernels' frame groups (FPW frames) past the first one per
// wavefront come from a u32 counter in the kSchedBytes just before their
// slices (polar_tree.hip, polar_lane.hpp); tree_launch / lane_launch zero it.
constexpr int kSchedBytes = 4096;
hipError_t tree_prepare(const TreeInfo& t, int* max_blocks_per_cu);
hipError_t tree_launch(const TreeInfo& t, const double* llr, int64_t ld, uint8_t* out, const uint32_t* frozen_dec,
                       const int32_t* info_pos, int64_t batch, int K, int Lsz, unsigned char* ws, int grid,
                       unsigned long long* stamps, const uint32_t* crc_g, const void* aux, hipStream_t s,
                       int ds_mode = 0);  // ds_mode 1 / 2 (PL_DIAG): the dead-store record / replay instance

// SCL frames with NaN path metrics (polar_nan.hip): the list kernels set bit f
// of masks[wave][pass] for frame f of that pass; polar_nan_redo_kernel decodes
// those frames again in the reference's candidate order.  A launch runs at most
// kNanMaskPasses passes of its persistent grid.
constexpr int kNanMaskPasses = 64;
constexpr int kMaxRedoList = 2048;  // the redo kernel's list state of one frame fits LDS up to here
// lists above kMaxRedoList keep that state in global scratch; list_size * N is
// bounded so that the kernel's int indices (path x element) stay below 2^31
constexpr int kMaxListSize = 1 << 16;
constexpr int64_t kMaxListTimesN = (int64_t)1 << 30;
// Bytes of the mask words of up to `grid` wavefronts, u64 [grid][kNanMaskPasses]
// (a multiple of 64 KB, at the start of a list plan's workspace).  They are zero
// between decodes: zeroed when the workspace is allocated, ORed by the list
// kernels, re-zeroed by the redo kernel after it reads them.
inline size_t nan_mask_region(int64_t grid) { return ((size_t)grid * 8 * kNanMaskPasses + 65535) / 65536 * 65536; }
size_t nan_redo_unit(int N, int list_size);  // scratch bytes per redo workgroup
int nan_redo_lds_bytes(int list_size);
hipError_t nan_redo_prepare(int list_size);
// path-metric evaluation of the list kernel whose frames are redone: the lane
// kernel's path_metrics (libm-style log1p(exp(-x))), or the tree instances'
// path_metrics_fast with the fused (n <= PL_METRIC_FUSED_NMAX) or lean form
enum RedoMetric { kRedoMetricLane = 0, kRedoMetricFused = 1, kRedoMetricLean = 2 };
hipError_t nan_redo_launch(const double* llr, int64_t ld, uint8_t* out, int64_t batch, int N, int K, int Lsz,
                           const uint32_t* frozen_dec, const int32_t* info_pos, const uint32_t* crc_g,
                           uint64_t* masks, int grid, int fpw, int metric, unsigned char* scratch,
                           size_t scratch_bytes, int max_blocks, hipStream_t s);

#if PL_DIAG
// frame-per-wavefront SCL N=1024 L=8 prototype (polar_fpw.hip, diagnostic build)
hipError_t fpw_launch(const double* llr, int64_t ld, uint8_t* out, const uint32_t* frozen_dec,
                      const int32_t* info_pos, int64_t batch, int K, unsigned long long* stamps, int grid,
                      hipStream_t st);
#endif

hipError_t polar_encode_launch(int N, int K, const int32_t* info_pos, const uint8_t* msg,
                               int64_t batch, uint8_t* cw, hipStream_t s);
hipError_t random_bits_launch(uint64_t seed, int64_t off, int64_t batch, int k, uint8_t* bits,
                              hipStream_t s);
hipError_t awgn_launch(const uint8_t* cw, int n, int64_t batch, double sigma, double sigma2,
                       uint64_t seed, int64_t off, double* llr, int64_t ld, hipStream_t s);
hipError_t rayleigh_launch(const uint8_t* cw, int n, int64_t batch, double sigma, double sigma2, uint64_t seed,
                           int64_t off, double* llr, int64_t ld, hipStream_t s);
hipError_t bsc_launch(const uint8_t* cw, int n, int64_t batch, double p, uint64_t seed, int64_t off, uint8_t* out,
                      int64_t ld, hipStream_t s);
hipError_t gf2_encode_launch(const uint32_t* g, int k, int n, const uint8_t* msg, int64_t ldm, int64_t batch,
                             uint8_t* cw, int64_t ldc, hipStream_t s);
hipError_t crc_append_launch(uint8_t* msg, int64_t ld, int64_t batch, int k_data, int crc_len, uint32_t poly,
                             hipStream_t s);
hipError_t count_errors_launch(const uint8_t* ref, int64_t ldr, const uint8_t* dec, int64_t ldd,
                               int width, int64_t batch, int64_t* counts, hipStream_t s);

// ---- LDPC (ldpc.hip); LdpcGeom / LdpcDev and the planner that fills them: ldpc_plan.hpp ----
hipError_t ldpc_launch(const LdpcGeom& g, const LdpcDev& d, const double* llr, int64_t ld,
                       uint8_t* bits, int32_t* iters, int64_t batch, double* work, hipStream_t s);
hipError_t ldpc_prepare(const LdpcGeom& g);
#if PL_DIAG
hipError_t ldpc_launch_stamped(const LdpcGeom& g, const LdpcDev& d, const double* llr, int64_t ld, uint8_t* bits,
                               int32_t* iters, int64_t batch, unsigned long long* stamps, hipStream_t s);
#endif

// ---- layered min-sum (ldpc_layered.hip); LmsGeom / LmsDev: ldpc_plan.hpp ----
hipError_t lms_prepare(const LmsGeom& g);
// post: fp64 [batch][ld_post] posteriors or null; work: [batch] state slices (use_global) or null
hipError_t lms_launch(const LmsGeom& g, const LmsDev& d, const double* llr, int64_t ld, uint8_t* bits, int32_t* iters,
                      double* post, int64_t ld_post, int64_t batch, unsigned char* work, hipStream_t s);

// ---- quasi-cyclic layered min-sum: one overload set over the geometry and the type of llr / post; the
// kernel behind all of them is ldpc_qc_frame.hpp's.  QcGeom, QcFixedGeom: ldpc_plan.hpp ----
// floating point (ldpc_qc_layered.hip).  f32: a single-precision plan (QcHostPlan::f32): the float
// instances, which take fp64 or fp32 llr / post
hipError_t qc_prepare(const QcGeom& g, bool f32);
// tab: the plan's layer stream (device); the other arguments as lms_launch
hipError_t qc_launch(const QcGeom& g, bool f32, const int32_t* tab, const double* llr, int64_t ld, uint8_t* bits,
                     int32_t* iters, double* post, int64_t ld_post, int64_t batch, unsigned char* work, hipStream_t s);
// fp32 llr and post: single-precision plans only (the caller checks)
hipError_t qc_launch(const QcGeom& g, const int32_t* tab, const float* llr, int64_t ld, uint8_t* bits, int32_t* iters,
                     float* post, int64_t ld_post, int64_t batch, unsigned char* work, hipStream_t s);

// int8 fixed point (ldpc_qc_fixed.hip): llr int8 [batch][ld]; post int8 [batch][ld_post] or null
hipError_t qc_prepare(const QcFixedGeom& g);
hipError_t qc_launch(const QcFixedGeom& g, const int32_t* tab, const int8_t* llr, int64_t ld, uint8_t* bits,
                     int32_t* iters, int8_t* post, int64_t ld_post, int64_t batch, unsigned char* work, hipStream_t s);

// fp64 sum-product (ldpc_qc_bp.hip): llr and post fp64, as the fp64 min-sum plan's
hipError_t qc_prepare(const QcBpGeom& g);
hipError_t qc_launch(const QcBpGeom& g, const int32_t* tab, const double* llr, int64_t ld, uint8_t* bits,
                     int32_t* iters, double* post, int64_t ld_post, int64_t batch, unsigned char* work, hipStream_t s);

// ---- the LLR quantiser (ldpc_qc_fixed.hip) ----
// llr [batch][ldi] double, or float with f32; out int8 [batch][ldo]; chunks its launches itself
hipError_t llr_quantize_launch(const void* llr, bool f32, int64_t ldi, int64_t batch, int n, double scale, int llr_max,
                               int8_t* out, int64_t ldo, hipStream_t s);

// ---- quasi-cyclic encoder from the base matrix (ldpc_qc_encode.hip); QcEncGeom: ldpc_plan.hpp ----
hipError_t qc_encode_prepare(const QcEncGeom& g);
// tab: the plan's stream (device); msg uint8 [batch][ldm] (bit 0 of each byte), cw uint8 [batch][ldc]
hipError_t qc_encode_launch(const QcEncGeom& g, const int32_t* tab, const uint8_t* msg, int64_t ldm, int64_t batch,
                            uint8_t* cw, int64_t ldc, hipStream_t s);

// ---- rate matching of quasi-cyclic codes (ldpc_qc_ratematch.hip); pl_rate_match: include/polarldpc.h ----
// rm: checked (rate_match_check).  cw uint8 [batch][ldc], e uint8 [batch][lde]; llr [batch][ldl] float or
// double, out [batch][ldo] float or double, pitches in elements.  Both chunk their launches themselves.
hipError_t rate_match_launch(const pl_rate_match& rm, const uint8_t* cw, int64_t ldc, int64_t batch, uint8_t* e,
                             int64_t lde, hipStream_t s);
hipError_t rate_recover_launch(const pl_rate_match& rm, const void* llr, int64_t ldl, bool llr_f32, int64_t batch,
                               void* out, int64_t ldo, bool out_f32, int n_out, double filler, bool acc,
                               hipStream_t s);

// ---- rate matching of polar codes (polar_ratematch.hip); pl_polar_rm: include/polarldpc.h ----
// rm: checked (pl_polar_rate_match_check).  cw uint8 [batch][ldc], e uint8 [batch][lde]; llr [batch][ldl] float
// or double, out double [batch][ldo], pitches in elements.  Both chunk their launches themselves.
hipError_t polar_rate_match_launch(const pl_polar_rm& rm, const uint8_t* cw, int64_t ldc, int64_t batch, uint8_t* e,
                                   int64_t lde, hipStream_t s);
hipError_t polar_rate_recover_launch(const pl_polar_rm& rm, const void* llr, int64_t ldl, bool llr_f32, int64_t batch,
                                     double* out, int64_t ldo, double known, bool acc, hipStream_t s);

// ---- Gray-mapped QAM (qam.hip); the definition: include/polarldpc.h, pl_qam_check ----
// m, E checked (qam_check), S and scale from it.  e uint8 [batch][lde] (null for awgn: all-zero bits); x, y
// double [batch][ld] of 2 S used elements; llr [batch][ldl] double or float; pitches in elements; w = 1 / (2
// sigma^2).  All chunk their launches themselves.
hipError_t qam_modulate_launch(int m, int64_t E, int64_t S, double scale, const uint8_t* e, int64_t lde, int64_t batch,
                               double* x, int64_t ldx, hipStream_t s);
hipError_t qam_awgn_launch(int m, int64_t E, int64_t S, double scale, const uint8_t* e, int64_t lde, int64_t batch,
                           double sigma, uint64_t seed, int64_t off, double* y, int64_t ldy, hipStream_t s);
hipError_t qam_demap_launch(int m, int64_t E, int64_t S, double scale, const double* y, int64_t ldy, int64_t batch,
                            double w, void* llr, int64_t ldl, bool llr_f32, hipStream_t s);
// Block Rayleigh fading (the definition: include/polarldpc.h, pl_qam_fading_check): m, E, Lc checked
// (qam_fading_check), S from it; h double [batch][ldh] of 2 Q used elements, Re and Im interleaved.
hipError_t qam_rayleigh_launch(int m, int64_t E, int64_t S, int64_t Lc, double scale, const uint8_t* e, int64_t lde,
                               int64_t batch, double sigma, uint64_t seed, int64_t off, double* y, int64_t ldy,
                               double* h, int64_t ldh, hipStream_t s);
hipError_t qam_demap_csi_launch(int m, int64_t E, int64_t S, int64_t Lc, double scale, const double* y, int64_t ldy,
                                const double* h, int64_t ldh, int64_t batch, double w, void* llr, int64_t ldl,
                                bool llr_f32, hipStream_t s);
// The exact log-MAP demapper (the definition: include/polarldpc.h, pl_qam_demap_logmap): qam_demap_launch's
// arguments with h == nullptr (Lc, ldh not used), qam_demap_csi_launch's otherwise.
hipError_t qam_demap_logmap_launch(int m, int64_t E, int64_t S, int64_t Lc, double scale, const double* y, int64_t ldy,
                                   const double* h, int64_t ldh, int64_t batch, double w, void* llr, int64_t ldl,
                                   bool llr_f32, hipStream_t s);

// ---- the bit interleaver (interleave.hip); the definition: include/polarldpc.h, pl_interleave_check ----
// kind, p checked (ilv_check).  e, f [batch][ld], pitches in elements: uint8 for the bits, double or float
// (f32) for the LLRs.  Frames of at most kIlvLdsBytes are permuted in LDS, longer ones directly in global
// memory.  Both chunk their launches themselves.
constexpr int64_t kIlvLdsBytes = 65536;
hipError_t bit_interleave_launch(int kind, const IlvParams& p, const uint8_t* e, int64_t lde, int64_t batch, uint8_t* f,
                                 int64_t ldf, hipStream_t s);
hipError_t llr_deinterleave_launch(int kind, const IlvParams& p, const void* f, int64_t ldf, int64_t batch, void* e,
                                   int64_t lde, bool f32, hipStream_t s);

}  // namespace pl

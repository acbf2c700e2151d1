// C-ABI of libpolarldpc.so (include/polarldpc.h): plan lifetime, argument
// checking (mirroring the reference's assertions), dispatch to the kernels.
#include "../../include/polarldpc.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "internal.hpp"
#include "qam_check.hpp"

// Device workspace of one stream (polar: per resident wavefront; LDPC codes
// whose messages exceed LDS: per frame of a chunk).  Grown lazily to the batch.
// Its own mutex serialises the decodes of that stream only, so a stream that
// drains and regrows its buffer never stalls decodes on other streams.
struct Workspace {
    std::mutex mu;
    void* ptr = nullptr;
    // written under `mu`; atomic so pl_plan_workspace_stats may read it under the map mutex only
    std::atomic<size_t> bytes{0};
    // after an out-of-memory fallback: the request that did not fit.  Later decodes
    // needing no more than it run on the smaller buffer (decode_impl clamps the grid)
    // instead of draining and retrying the allocation every call; pl_plan_reserve,
    // or a larger request, retries.
    size_t failed_need = 0;
    // Wait for the work queued on the buffer's stream (it may still read the buffer), then free
    // it.  The buffer is gone whatever the wait returns; the caller reports that status.
    hipError_t drain(hipStream_t s) {
        const hipError_t e = hipStreamSynchronize(s);
        hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
        return e;
    }
    ~Workspace() {
        if (ptr) hipFree(ptr);  // hipFree waits for work that still uses it
    }
};

struct pl_plan {
    int kind = 0;  // 0 polar, 1 ldpc
    int device = 0;
    // polar
    pl::PolarGeom pg{};  // N, K, F, lds_bytes of the chosen kernel
    bool sc = false;
    int list_size = 0;
    uint32_t* d_frozen_dec = nullptr;  // decode-order frozen bitmask [ceil(N/32)]
    int32_t* d_info_pos = nullptr;     // [K] ascending info indices
    uint32_t* d_crc_g = nullptr;       // CA-SCL: CRC contribution of x_hat bit j [N] (null = plain SCL)
    uint32_t* d_r0k = nullptr;         // SC tree kernel: log2 size of the largest all-frozen node at leaf i (4-bit fields)
    std::vector<int32_t> h_info;       // ascending info positions (host copy)
    bool tree = false;      // compile-time-geometry kernel (polar_tree.hip); else polar_lane.hip
    pl::TreeInfo tinfo{};
    // the small-batch tree instance (polar_tree.hip tree_table_small): used for a
    // decode whose wavefronts all fit the device at its occupancy, small_grid_max
    bool tree_small = false;
    pl::TreeInfo tinfo_small{};
    int small_grid_max = 0;
    pl::LaneGeom lgeo{};
    int fpw = 1;            // frames per wavefront
    int lane_grid_max = 0;  // resident wavefronts (persistent grid)
    // false: the lane kernel's geometry needs more LDS than the device has (SC and
    // list 1 at N = 32768: 64 frames' final transforms, 256 KiB).  The plan then
    // serves pl_polar_encode only; decodes return PL_EUNSUPPORTED.
    bool decodable = true;
    // ldpc
    pl::LdpcGeom lg{};
    pl::LdpcDev ld{};
    int32_t* d_ldpc = nullptr;
    int64_t ldpc_chunk = 16384;  // frames per launch of the global-workspace kernel
    // layered min-sum (ldpc_layered.hip): kind 1 with its own geometry; lg.n is set too
    bool layered = false;
    pl::LmsGeom lms{};
    pl::LmsDev lmsd{};
    // quasi-cyclic layered min-sum (ldpc_qc_layered.hip): a layered plan (lms.n, lms.m set) whose
    // kernel geometry is qcg and whose table buffer is the layer stream
    bool qc = false;
    bool qc_f32 = false;  // created with PL_LDPC_QC_F32: state and arithmetic in single precision
    pl::QcGeom qcg{};
    // int8 fixed-point quasi-cyclic layered min-sum (ldpc_qc_fixed.hip): a layered plan (lms.n, lms.m set)
    // that only pl_ldpc_decode_i8 decodes; its table buffer is the layer stream
    bool qc_fixed = false;
    pl::QcFixedGeom qfg{};
    // fp64 quasi-cyclic layered sum-product (ldpc_qc_bp.hip): a layered plan (lms.n, lms.m set) decoded
    // through the fp64 entry points; its table buffer is the layer stream
    bool qc_bp = false;
    pl::QcBpGeom qbg{};
    // workspace: bytes per unit (polar: one resident wave; LDPC global: one
    // frame), one buffer per stream (plans are shared across host threads that
    // use distinct streams; a decode only ever touches its stream's buffer)
    size_t ws_unit = 0;
    // polar list decoders: NaN-frame masks (kNanMaskPasses u64 per resident
    // wavefront, at the start of the workspace) and the scratch one workgroup of
    // polar_nan_redo_kernel needs (it reuses the list kernel's slices after it)
    size_t mask_bytes = 0, redo_unit = 0;
    size_t head_bytes = 0;  // polar: NaN masks + the tree kernel's frame-group counter, before the slices
    bool generic = false;  // list_size > 1024: polar_nan.hip decodes every frame
    int redo_blocks = 0;
    std::mutex mu;  // guards the map only; each entry has its own mutex
    std::unordered_map<hipStream_t, std::shared_ptr<Workspace>> ws;
};

static thread_local std::string g_err;

// HIP caps a launch at 2^32 work-items per grid dimension; per-frame kernels
// (one workgroup per frame) are launched in chunks below 2^31 work-items.
constexpr int64_t kMaxLaunchItems = 1LL << 31;

static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
static int hipfail(hipError_t e, const char* what) {
    // the runtime keeps a failed call's code as its "last error": taken here, so that
    // the caller's next launch (torch checks it after each of its own) does not report it
    (void)hipGetLastError();
    return fail(e == hipErrorOutOfMemory ? PL_ENOMEM : PL_EHIP,
                std::string(what) + ": " + hipGetErrorString(e));
}

extern "C" const char* pl_last_error(void) { return g_err.c_str(); }

static int bitrev(int v, int nb) {
    int r = 0;
    for (int i = 0; i < nb; ++i) { r = (r << 1) | (v & 1); v >>= 1; }
    return r;
}

template <typename T>
static hipError_t upload(T** dst, const std::vector<T>& src) {
    const size_t bytes = (src.empty() ? 1 : src.size()) * sizeof(T);
    hipError_t e = hipMalloc((void**)dst, bytes);
    if (e != hipSuccess) return e;
    if (!src.empty()) e = hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice);
    return e;
}

static int env_int(const char* name, int dflt) {
    const char* s = std::getenv(name);
    return (s && *s) ? std::atoi(s) : dflt;
}

// Every call that touches a plan's device memory must run on the plan's device
// (the one current at plan creation): a workspace allocated, or a kernel
// launched, on another device would use foreign pointers.  The same holds for
// an encoder; `whose`: "plan's" or "encoder's".
static int check_device(int device, const char* whose) {
    int cur = -1;
    const hipError_t e = hipGetDevice(&cur);
    if (e != hipSuccess) return hipfail(e, "hipGetDevice");
    if (cur != device)
        return fail(PL_EINVAL, "current device " + std::to_string(cur) + " is not the " + whose + " device " +
                                   std::to_string(device) + " (hipSetDevice first)");
    return PL_OK;
}
static int check_device(const pl_plan* p) { return check_device(p->device, "plan's"); }

// A plan or an encoder under construction: destroyed on every return that does not release() it into *out.
template <class T, int (*Destroy)(T*)>
struct Destroyer {
    void operator()(T* t) const { Destroy(t); }
};
using PlanPtr = std::unique_ptr<pl_plan, Destroyer<pl_plan, pl_plan_destroy>>;

// fn(b0, nb) on consecutive chunks of at most `step` frames; stops at the first status that is not PL_OK.
template <class F>
static int for_chunks(int64_t batch, int64_t step, F&& fn) {
    for (int64_t b0 = 0; b0 < batch; b0 += step)
        if (const int rc = fn(b0, std::min<int64_t>(step, batch - b0))) return rc;
    return PL_OK;
}

// the metric evaluation of the list kernel a plan's NaN frames come from (polar_nan.hip)
static int redo_metric(const pl_plan* p) {
    if (!p->tree && !p->generic) return pl::kRedoMetricLane;
    return p->pg.N <= (1 << PL_METRIC_FUSED_NMAX) ? pl::kRedoMetricFused : pl::kRedoMetricLean;
}

static int device_cus(int dev) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        return prop.multiProcessorCount;
    return 256;
}

extern "C" int pl_polar_plan_create(int32_t N, int32_t K, const uint8_t* frozen_mask, int32_t list_size,
                                    int32_t flags, pl_plan** out) {
    if (!out) return fail(PL_EINVAL, "out is NULL");
    *out = nullptr;
    if (N < 2 || (N & (N - 1)) || N > (1 << pl::kMaxDepth))
        return fail(PL_EINVAL, "N must be a power of 2 in [2, 32768]");
    if (!(0 < K && K <= N)) return fail(PL_EINVAL, "K (info positions) must be in [1, N]");
    if (list_size < 0) return fail(PL_EINVAL, "list_size must be >= 1 (0 = SC)");
    if (list_size > pl::kMaxListSize || (int64_t)list_size * N > pl::kMaxListTimesN)
        return fail(PL_EUNSUPPORTED, "list_size > 65536 or list_size * N > 2^30 not supported by this build");
    if (!frozen_mask) return fail(PL_EINVAL, "frozen_mask is NULL");
    int n = 0;
    while ((1 << n) < N) ++n;
    std::vector<int32_t> info;
    for (int j = 0; j < N; ++j)
        if (!frozen_mask[j]) info.push_back(j);
    if ((int)info.size() != K) return fail(PL_EINVAL, "number of unfrozen positions != K");
    std::vector<uint32_t> fdec((N + 31) / 32, 0u);
    for (int i = 0; i < N; ++i)
        if (frozen_mask[bitrev(i, n)]) fdec[i >> 5] |= 1u << (i & 31);

    PlanPtr plan(new pl_plan());
    pl_plan* const p = plan.get();
    p->kind = 0;
    p->h_info = info;
    p->sc = (list_size == 0);
    p->list_size = list_size;
    hipGetDevice(&p->device);
    const char* kern = std::getenv("PL_POLAR_KERNEL");
    int lcap = 1;
    while (lcap < (p->sc ? 1 : list_size)) lcap <<= 1;
    // lists above 1024 (one frame per workgroup no longer holds one lane per
    // path): every frame through the exact single-workgroup decoder of polar_nan.hip
    p->generic = list_size > 1024;
    p->tree = !p->generic && !(kern && std::string(kern) == "lane") && !(flags & 0x3F) &&
              pl::tree_lookup(n, lcap, p->sc, &p->tinfo);
    hipError_t e;
    if ((e = upload(&p->d_frozen_dec, fdec)) != hipSuccess || (e = upload(&p->d_info_pos, info)) != hipSuccess)
        return hipfail(e, "plan upload");
    p->pg.N = N;
    p->pg.K = K;
    if (p->tree && p->sc) {
        // r0k[i] (decode order): the largest k with i a multiple of 2^k (any k
        // for i = 0) and leaves i .. i + 2^k - 1 all frozen.  K >= 1 info bits,
        // so k < n <= 15: eight 4-bit fields per word, which the kernel reads
        // with scalar loads.
        std::vector<uint32_t> r0k((size_t)(N + 7) / 8, 0u);
        for (int i = 0; i < N; ++i) {
            int k = 0;
            while (k + 1 < n + 1 && (i & ((1 << (k + 1)) - 1)) == 0 && i + (1 << (k + 1)) <= N) {
                bool all = true;
                for (int t = i; t < i + (1 << (k + 1)) && all; ++t) all = (fdec[t >> 5] >> (t & 31)) & 1u;
                if (!all) break;
                ++k;
            }
            r0k[(size_t)i >> 3] |= (uint32_t)k << (4 * (i & 7));
        }
        if ((e = upload(&p->d_r0k, r0k)) != hipSuccess)
            return hipfail(e, "plan upload");
    }
    int per_cu = 1;
    if (p->generic) {
        p->pg.F = 0;
        p->pg.lds_bytes = pl::nan_redo_lds_bytes(list_size);
        p->fpw = 1;
        p->ws_unit = 0;
        e = hipSuccess;
    } else if (p->tree) {
        p->pg.F = p->tinfo.F;
        p->pg.lds_bytes = p->tinfo.lds_bytes;
        p->fpw = p->tinfo.fpw;
        p->ws_unit = (size_t)p->tinfo.ws_bytes;
        e = pl::tree_prepare(p->tinfo, &per_cu);
    } else {
        // lane-per-path kernel for every (N, L) without a tree instance; flags
        // bits 0..3 pick its fused-top depth (diagnostic), 0x10 / 0x20 force it
        int F = flags & 0xF;
        if (!F) F = env_int("PL_POLAR_FUSED", 3);
        pl::lane_geom(N, K, p->sc ? 1 : list_size, F, env_int("PL_POLAR_LDS_BUDGET", 8 * 1024), &p->lgeo);
        p->pg.F = p->lgeo.F;
        p->pg.lds_bytes = p->lgeo.lds_bytes;
        p->fpw = p->lgeo.lcap >= 64 ? 1 : 64 / p->lgeo.lcap;
        p->ws_unit = (size_t)p->lgeo.ws_bytes;
        int optin = 0;
        e = hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, p->device);
        if (e == hipSuccess) {
            p->decodable = p->lgeo.lds_bytes <= optin;
            if (p->decodable) e = pl::lane_prepare(p->lgeo, p->sc, &per_cu);
        }
    }
    if (e != hipSuccess)
        return hipfail(e, "polar kernel prepare");
    p->lane_grid_max = per_cu * device_cus(p->device);
    const int waves_env = env_int("PL_POLAR_WAVES", 0);
    if (waves_env > 0) p->lane_grid_max = waves_env;
    if (p->tree && waves_env <= 0 && pl::tree_lookup_small(n, lcap, p->sc, &p->tinfo_small) &&
        p->tinfo_small.ws_bytes <= p->tinfo.ws_bytes && p->tinfo_small.fpw == p->fpw) {
        // its slices fit the main instance's (the workspace is sized for that one)
        int per_cu_small = 0;
        if ((e = pl::tree_prepare(p->tinfo_small, &per_cu_small)) != hipSuccess)
            return hipfail(e, "polar kernel prepare");
        p->small_grid_max = std::min(per_cu_small * device_cus(p->device), p->lane_grid_max);
        p->tree_small = p->small_grid_max > 0;
    }
    if (!p->sc) {
        p->mask_bytes = p->generic ? 0 : pl::nan_mask_region(p->lane_grid_max);
        p->redo_unit = pl::nan_redo_unit(N, list_size);
        p->redo_blocks = device_cus(p->device);
        if (p->generic) {  // scratch of up to 2 GB (at least one frame's): a 2048-path list of N = 1024 holds 23 MB
            // one frame's list state must fit the device (list_size * N = 2^30 needs ~11 GB)
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && p->redo_unit > total_b)
                return fail(PL_EUNSUPPORTED, "list_size: one frame's list state exceeds this device's memory");
            const size_t cap = (size_t)2 << 30;
            p->redo_blocks = (int)std::max<size_t>(1, std::min<size_t>((size_t)p->redo_blocks, cap / p->redo_unit));
            p->lane_grid_max = p->redo_blocks;
        }
        // the redo kernel's dynamic-LDS limit (a per-function attribute) raised to this list's need;
        // a list whose state does not fit the device's LDS is refused here, so that any error
        // of the prepare call itself is a HIP error
        int optin = 0;
        if ((e = hipDeviceGetAttribute(&optin, hipDeviceAttributeSharedMemPerBlockOptin, p->device)) != hipSuccess)
            return hipfail(e, "device attribute query");
        if (pl::nan_redo_lds_bytes(list_size) > optin)
            return fail(PL_EUNSUPPORTED, "list_size: the redo kernel's list state exceeds this device's LDS");
        if ((e = pl::nan_redo_prepare(list_size)) != hipSuccess)
            return hipfail(e, "NaN redo kernel prepare");
    }
    p->head_bytes = p->mask_bytes + (p->generic ? 0 : (size_t)pl::kSchedBytes);
    *out = plan.release();
    return PL_OK;
}

// The LDPC planning switches (ldpc_plan.hpp; the planner itself reads no
// environment).  The check kernel exists in the diagnostic build only; a
// frames-per-workgroup request other than 1 means 2.
static_assert(PL_LDPC_KERNEL_DEFAULT == pl::kLdpcKernelDefault && PL_LDPC_KERNEL_GENERIC == pl::kLdpcKernelGeneric &&
              PL_LDPC_KERNEL_REG == pl::kLdpcKernelReg && PL_LDPC_KERNEL_COMPACT == pl::kLdpcKernelCompact &&
              PL_LDPC_KERNEL_CHECK == pl::kLdpcKernelCheck, "include/polarldpc.h numbers the overrides as ldpc_plan.hpp");
static pl::LdpcPlanOptions ldpc_options(int kernel, int bp_fpg, int lms_global) {
    pl::LdpcPlanOptions o;
    o.kernel = (kernel == pl::kLdpcKernelCheck && !PL_DIAG) ? pl::kLdpcKernelDefault : kernel;
    o.bp_fpg = bp_fpg == 0 ? 0 : (bp_fpg == 1 ? 1 : 2);
    o.lms_global = lms_global != 0;
    return o;
}
// PL_LDPC_KERNEL, PL_BP_FPG and PL_LMS_GLOBAL: the one place that reads them
static pl::LdpcPlanOptions ldpc_env_options() {
    const char* lk = std::getenv("PL_LDPC_KERNEL");
    const std::string k = lk ? lk : "";
    const char* fpg = std::getenv("PL_BP_FPG");
    return ldpc_options(k == "generic" ? pl::kLdpcKernelGeneric : k == "reg" ? pl::kLdpcKernelReg
                        : k == "compact" ? pl::kLdpcKernelCompact : k == "check" ? pl::kLdpcKernelCheck
                                                                                 : pl::kLdpcKernelDefault,
                        (fpg && *fpg) ? (std::atoi(fpg) == 1 ? 1 : 2) : 0, env_int("PL_LMS_GLOBAL", 0));
}

// An LDPC plan object around the planner's tables, uploaded as one device buffer.
static int ldpc_plan_upload(const std::vector<int32_t>& tables, PlanPtr* plan) {
    pl_plan* const p = new pl_plan();
    plan->reset(p);
    p->kind = 1;
    hipGetDevice(&p->device);
    p->ldpc_chunk = std::max(1, env_int("PL_LDPC_CHUNK", 16384));
    const hipError_t e = upload(&p->d_ldpc, tables);
    return e == hipSuccess ? PL_OK : hipfail(e, "plan upload");
}

extern "C" int pl_ldpc_plan_create(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx,
                                   int32_t algo, int32_t max_iter, int32_t early_stop, double normalization,
                                   int32_t flags, pl_plan** out) {
    (void)flags;
    if (!out) return fail(PL_EINVAL, "out is NULL");
    *out = nullptr;
    // every argument check (ldpc_plan.cpp) comes before the first device call
    pl::LdpcHostPlan hp;
    const pl::PlanStatus st =
        pl::ldpc_plan_build(m, n, row_ptr, col_idx, algo, max_iter, early_stop, normalization, ldpc_env_options(), &hp);
    if (st.code) return fail(st.code, st.msg);
    PlanPtr plan;
    if (int rc = ldpc_plan_upload(hp.tables, &plan)) return rc;
    pl_plan* const p = plan.get();
    p->lg = hp.geom;
    p->ld = hp.dev(p->d_ldpc);
    const hipError_t e = pl::ldpc_prepare(p->lg);
    if (e != hipSuccess) return hipfail(e, "hipFuncSetAttribute");
    p->ws_unit = pl::ldpc_work_bytes_per_frame(p->lg);
    *out = plan.release();
    return PL_OK;
}

extern "C" int pl_ldpc_layered_plan_create(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx,
                                           int32_t n_layers, const int32_t* layer_ptr, const int32_t* layer_rows,
                                           int32_t max_iter, int32_t early_stop, double normalization, int32_t flags,
                                           pl_plan** out) {
    (void)flags;
    if (!out) return fail(PL_EINVAL, "out is NULL");
    *out = nullptr;
    // every argument check (ldpc_plan.cpp) comes before the first device call
    pl::LmsHostPlan hp;
    const pl::PlanStatus st = pl::lms_plan_build(m, n, row_ptr, col_idx, n_layers, layer_ptr, layer_rows, max_iter,
                                                 early_stop, normalization, ldpc_env_options(), &hp);
    if (st.code) return fail(st.code, st.msg);
    PlanPtr plan;
    if (int rc = ldpc_plan_upload(hp.tables, &plan)) return rc;
    pl_plan* const p = plan.get();
    p->layered = true;
    p->lg.n = n; p->lg.m = m; p->lg.E = hp.geom.E;
    p->lms = hp.geom;
    p->lmsd = hp.dev(p->d_ldpc);
    const hipError_t e = pl::lms_prepare(p->lms);
    if (e != hipSuccess) return hipfail(e, "hipFuncSetAttribute");
    p->ws_unit = p->lms.use_global ? (size_t)p->lms.state_bytes : 0;
    *out = plan.release();
    return PL_OK;
}

extern "C" int pl_ldpc_qc_plan_create(int32_t mb, int32_t nb, int32_t z, const int32_t* shift,
                                      const int32_t* layer_order, int32_t max_iter, int32_t early_stop,
                                      double normalization, int32_t flags, pl_plan** out) {
    if (!out) return fail(PL_EINVAL, "out is NULL");
    *out = nullptr;
    // every argument check (ldpc_plan.cpp) comes before the first device call
    pl::QcHostPlan hp;
    pl::LdpcPlanOptions opt = ldpc_env_options();
    if (flags & PL_LDPC_QC_F32) opt.qc_state_elem = 4;  // the other bits are ignored
    const pl::PlanStatus st = pl::qc_plan_build(mb, nb, z, shift, layer_order, max_iter, early_stop, normalization,
                                                opt, &hp);
    if (st.code) return fail(st.code, st.msg);
    PlanPtr plan;
    if (int rc = ldpc_plan_upload(hp.tables, &plan)) return rc;
    pl_plan* const p = plan.get();
    p->layered = true;
    p->qc = true;
    p->qcg = hp.geom;
    p->qc_f32 = hp.f32;
    p->lg.n = p->lms.n = hp.geom.n;
    p->lg.m = p->lms.m = hp.geom.m;
    const hipError_t e = pl::qc_prepare(p->qcg, p->qc_f32);
    if (e != hipSuccess) return hipfail(e, "hipFuncSetAttribute");
    p->ws_unit = p->qcg.use_global ? (size_t)p->qcg.state_bytes : 0;
    *out = plan.release();
    return PL_OK;
}

extern "C" int pl_ldpc_qc_fixed_plan_create(int32_t mb, int32_t nb, int32_t z, const int32_t* shift,
                                            const int32_t* layer_order, int32_t max_iter, int32_t early_stop,
                                            int32_t norm16, int32_t llr_max, int32_t msg_max, pl_plan** out) {
    if (!out) return fail(PL_EINVAL, "out is NULL");
    *out = nullptr;
    // every argument check (ldpc_plan.cpp) comes before the first device call
    pl::QcFixedHostPlan hp;
    const pl::PlanStatus st = pl::qc_fixed_plan_build(mb, nb, z, shift, layer_order, max_iter, early_stop, norm16,
                                                      llr_max, msg_max, ldpc_env_options(), &hp);
    if (st.code) return fail(st.code, st.msg);
    PlanPtr plan;
    if (int rc = ldpc_plan_upload(hp.tables, &plan)) return rc;
    pl_plan* const p = plan.get();
    p->layered = true;
    p->qc_fixed = true;
    p->qfg = hp.geom;
    p->lg.n = p->lms.n = hp.geom.n;
    p->lg.m = p->lms.m = hp.geom.m;
    const hipError_t e = pl::qc_prepare(p->qfg);
    if (e != hipSuccess) return hipfail(e, "hipFuncSetAttribute");
    p->ws_unit = p->qfg.use_global ? (size_t)p->qfg.state_bytes : 0;
    *out = plan.release();
    return PL_OK;
}

extern "C" int pl_ldpc_qc_bp_plan_create(int32_t mb, int32_t nb, int32_t z, const int32_t* shift,
                                         const int32_t* layer_order, int32_t max_iter, int32_t early_stop,
                                         double clip, pl_plan** out) {
    if (!out) return fail(PL_EINVAL, "out is NULL");
    *out = nullptr;
    // every argument check (ldpc_plan.cpp) comes before the first device call
    pl::QcBpHostPlan hp;
    const pl::PlanStatus st = pl::qc_bp_plan_build(mb, nb, z, shift, layer_order, max_iter, early_stop, clip,
                                                   ldpc_env_options(), &hp);
    if (st.code) return fail(st.code, st.msg);
    PlanPtr plan;
    if (int rc = ldpc_plan_upload(hp.tables, &plan)) return rc;
    pl_plan* const p = plan.get();
    p->layered = true;
    p->qc_bp = true;
    p->qbg = hp.geom;
    p->lg.n = p->lms.n = hp.geom.n;
    p->lg.m = p->lms.m = hp.geom.m;
    const hipError_t e = pl::qc_prepare(p->qbg);
    if (e != hipSuccess) return hipfail(e, "hipFuncSetAttribute");
    p->ws_unit = p->qbg.use_global ? (size_t)p->qbg.state_bytes : 0;
    *out = plan.release();
    return PL_OK;
}

// The planner's decisions for a code, with no plan object and no device call.
extern "C" int pl_debug_ldpc_plan_probe(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx,
                                        int32_t algo, int32_t max_iter, int32_t early_stop, double normalization,
                                        int32_t kernel_override, int32_t bp_fpg, int32_t lms_global,
                                        pl_ldpc_plan_probe* out) {
    if (!out) return fail(PL_EINVAL, "out is NULL");
    if (kernel_override < 0 || kernel_override > PL_LDPC_KERNEL_CHECK) return fail(PL_EINVAL, "bad kernel_override");
    pl::LdpcHostPlan hp;
    const pl::PlanStatus st = pl::ldpc_plan_build(m, n, row_ptr, col_idx, algo, max_iter, early_stop, normalization,
                                                  ldpc_options(kernel_override, bp_fpg, lms_global), &hp);
    if (st.code) return fail(st.code, st.msg);
    const pl::LdpcGeom& g = hp.geom;
    *out = pl_ldpc_plan_probe{pl::ldpc_kernel_code(g), g.threads, g.lds_bytes, g.use_global, g.reg_variant, g.grp,
                              g.fpg, g.tl, g.npad, g.compact, g.ms36, (int64_t)pl::ldpc_work_bytes_per_frame(g),
                              (int64_t)hp.tables.size(), (int64_t)hp.at.grp_meta, (int64_t)hp.at.ms_vw,
                              pl::plan_tables_digest(hp.tables)};
    return PL_OK;
}

extern "C" int pl_debug_ldpc_layered_plan_probe(int32_t m, int32_t n, const int32_t* row_ptr, const int32_t* col_idx,
                                                int32_t n_layers, const int32_t* layer_ptr, const int32_t* layer_rows,
                                                int32_t max_iter, int32_t early_stop, double normalization,
                                                int32_t kernel_override, int32_t bp_fpg, int32_t lms_global,
                                                pl_ldpc_layered_plan_probe* out) {
    if (!out) return fail(PL_EINVAL, "out is NULL");
    pl::LmsHostPlan hp;
    const pl::PlanStatus st = pl::lms_plan_build(m, n, row_ptr, col_idx, n_layers, layer_ptr, layer_rows, max_iter,
                                                 early_stop, normalization,
                                                 ldpc_options(kernel_override, bp_fpg, lms_global), &hp);
    if (st.code) return fail(st.code, st.msg);
    const pl::LmsGeom& g = hp.geom;
    *out = pl_ldpc_layered_plan_probe{pl::lms_kernel_code(g), g.maxdc, g.n_layers, g.max_layer, g.mw, g.wave,
                                      g.use_global, g.fpb, g.threads, g.lds_bytes, g.state_bytes, g.off_mm, g.off_meta,
                                      (int64_t)hp.tables.size(), pl::plan_tables_digest(hp.tables)};
    return PL_OK;
}

extern "C" int pl_debug_ldpc_qc_plan_probe_flags(int32_t mb, int32_t nb, int32_t z, const int32_t* shift,
                                                 const int32_t* layer_order, int32_t max_iter, int32_t early_stop,
                                                 double normalization, int32_t lms_global, int32_t flags,
                                                 pl_ldpc_qc_plan_probe* out) {
    if (!out) return fail(PL_EINVAL, "out is NULL");
    pl::QcHostPlan hp;
    pl::LdpcPlanOptions opt = ldpc_options(0, 0, lms_global);
    if (flags & PL_LDPC_QC_F32) opt.qc_state_elem = 4;
    const pl::PlanStatus st = pl::qc_plan_build(mb, nb, z, shift, layer_order, max_iter, early_stop, normalization,
                                                opt, &hp);
    if (st.code) return fail(st.code, st.msg);
    const pl::QcGeom& g = hp.geom;
    *out = pl_ldpc_qc_plan_probe{pl::qc_kernel_code(g, hp.f32), g.z, g.mb, g.nb, g.maxdc, g.dcap, g.mw, g.fpw, g.fpb,
                                 g.threads, g.lds_bytes, g.use_global, g.state_bytes, (int64_t)hp.tables.size(),
                                 pl::plan_tables_digest(hp.tables)};
    return PL_OK;
}

extern "C" int pl_debug_ldpc_qc_plan_probe(int32_t mb, int32_t nb, int32_t z, const int32_t* shift,
                                           const int32_t* layer_order, int32_t max_iter, int32_t early_stop,
                                           double normalization, int32_t lms_global, pl_ldpc_qc_plan_probe* out) {
    return pl_debug_ldpc_qc_plan_probe_flags(mb, nb, z, shift, layer_order, max_iter, early_stop, normalization,
                                             lms_global, 0, out);
}

extern "C" int pl_debug_ldpc_qc_fixed_plan_probe(int32_t mb, int32_t nb, int32_t z, const int32_t* shift,
                                                 const int32_t* layer_order, int32_t max_iter, int32_t early_stop,
                                                 int32_t norm16, int32_t llr_max, int32_t msg_max, int32_t lms_global,
                                                 pl_ldpc_qc_fixed_plan_probe* out) {
    if (!out) return fail(PL_EINVAL, "out is NULL");
    pl::QcFixedHostPlan hp;
    const pl::PlanStatus st = pl::qc_fixed_plan_build(mb, nb, z, shift, layer_order, max_iter, early_stop, norm16,
                                                      llr_max, msg_max, ldpc_options(0, 0, lms_global), &hp);
    if (st.code) return fail(st.code, st.msg);
    const pl::QcFixedGeom& g = hp.geom;
    *out = pl_ldpc_qc_fixed_plan_probe{pl::qc_fixed_kernel_code(g), g.z, g.mb, g.nb, g.maxdc, g.dcap, g.mw, g.fpw,
                                       g.fpb, g.threads, g.lds_bytes, g.use_global, g.norm16, g.llr_max, g.msg_max,
                                       0, g.state_bytes, g.off_p, (int64_t)hp.tables.size(),
                                       pl::plan_tables_digest(hp.tables)};
    return PL_OK;
}

extern "C" int pl_debug_ldpc_qc_bp_plan_probe(int32_t mb, int32_t nb, int32_t z, const int32_t* shift,
                                              const int32_t* layer_order, int32_t max_iter, int32_t early_stop,
                                              double clip, int32_t lms_global, pl_ldpc_qc_bp_plan_probe* out) {
    if (!out) return fail(PL_EINVAL, "out is NULL");
    pl::QcBpHostPlan hp;
    const pl::PlanStatus st = pl::qc_bp_plan_build(mb, nb, z, shift, layer_order, max_iter, early_stop, clip,
                                                   ldpc_options(0, 0, lms_global), &hp);
    if (st.code) return fail(st.code, st.msg);
    const pl::QcBpGeom& g = hp.geom;
    *out = pl_ldpc_qc_bp_plan_probe{pl::qc_bp_kernel_code(g), g.z, g.mb, g.nb, g.maxdc, g.dcap, g.mw, g.fpw, g.fpb,
                                    g.threads, g.lds_bytes, g.use_global, g.clip, g.state_bytes, g.off_r,
                                    (int64_t)hp.tables.size(), pl::plan_tables_digest(hp.tables)};
    return PL_OK;
}

// Polar workspace layout for a grid of `grid` resident wavefronts: a list
// plan's NaN masks first (for its largest grid, so they stay in place, and
// zero, from one decode to the next), then the tree / lane kernel's frame-group
// counter (zeroed by tree_launch / lane_launch before each launch), then the list kernel's
// slices, which the NaN redo kernel reuses as its scratch once the list kernel
// is done.
static size_t polar_bytes(const pl_plan* p, int64_t grid) {
    return p->head_bytes + std::max<size_t>(p->ws_unit * (size_t)grid, p->redo_unit);
}
// the smallest workspace a decode can run on (one wavefront's slice)
static size_t ws_min(const pl_plan* p) {
    if (p->kind == 0 && p->generic) return p->redo_unit;
    return p->kind == 0 ? polar_bytes(p, 1) : p->ws_unit;
}

// Workspace bytes a decode of `batch` frames uses at full speed.
static size_t ws_need(const pl_plan* p, int64_t batch) {
    if (batch <= 0 || (p->ws_unit == 0 && p->redo_unit == 0)) return 0;
    if (p->kind == 0 && p->generic) return p->redo_unit * (size_t)std::min<int64_t>(batch, p->redo_blocks);
    if (p->kind == 0) {
        const int64_t waves = (batch + p->fpw - 1) / p->fpw;
        return polar_bytes(p, std::min<int64_t>(waves, p->lane_grid_max));
    }
    return p->ws_unit * (size_t)std::min<int64_t>(batch, p->ldpc_chunk);
}

// Diagnostic-build options of one decode call (none in the product entry points):
// stamps = the tree kernel's stamp buffer (or, with ds_mode 1 / 2, the dead-store
// record / replay bitmask); flagged = a host array of `batch` bytes that receives,
// per frame, whether the list kernel flagged it for the NaN-order redo decoder.
struct DecodeDiag {
    unsigned long long* stamps = nullptr;
    int ds_mode = 0;
    uint8_t* flagged = nullptr;
};

// Layered min-sum decode; post ([batch][ld_post]) may be null.  LDS-resident
// state: launches below the grid limit; workspace-resident: chunks of the frames
// the workspace holds (one state slice per frame of a chunk).  IO: double; float on a
// quasi-cyclic plan made with PL_LDPC_QC_F32; int8_t on a fixed-point plan (pl_ldpc_decode_f32
// and pl_ldpc_decode_i8 check that).
template <typename IO>
static int lms_decode_impl(pl_plan* p, const IO* llr, int64_t batch, int64_t ld, uint8_t* bits, int32_t* iters,
                           IO* post, int64_t ld_post, void* ws, size_t ws_bytes, hipStream_t s) {
    constexpr bool kFixed = std::is_same<IO, int8_t>::value;
    if (p->ws_unit > 0 && (ws == nullptr || ws_bytes < p->ws_unit))
        return fail(PL_EINVAL, "workspace smaller than one unit (pl_plan_workspace_bytes)");
    if (kFixed && p->ws_unit > 0 && ((uintptr_t)ws & 15))
        return fail(PL_EINVAL, "workspace must be aligned to 16 bytes");
    const int64_t step = p->ws_unit > 0 ? std::min<int64_t>(p->ldpc_chunk, (int64_t)(ws_bytes / p->ws_unit))
                                        : kMaxLaunchItems / 1024;
    return for_chunks(batch, step, [&](int64_t b0, int64_t nb) {
        uint8_t* const bo = bits + b0 * p->lms.n;
        int32_t* const io = iters ? iters + b0 : nullptr;
        IO* const po = post ? post + b0 * ld_post : nullptr;
        hipError_t e;
        if constexpr (kFixed) {
            e = pl::qc_launch(p->qfg, p->d_ldpc, llr + b0 * ld, ld, bo, io, po, ld_post, nb, (unsigned char*)ws, s);
        } else if constexpr (std::is_same<IO, float>::value) {
            e = pl::qc_launch(p->qcg, p->d_ldpc, llr + b0 * ld, ld, bo, io, po, ld_post, nb, (unsigned char*)ws, s);
        } else {
            if (p->qc_bp)
                e = pl::qc_launch(p->qbg, p->d_ldpc, llr + b0 * ld, ld, bo, io, po, ld_post, nb, (unsigned char*)ws, s);
            else
                e = p->qc ? pl::qc_launch(p->qcg, p->qc_f32, p->d_ldpc, llr + b0 * ld, ld, bo, io, po, ld_post, nb,
                                          (unsigned char*)ws, s)
                          : pl::lms_launch(p->lms, p->lmsd, llr + b0 * ld, ld, bo, io, po, ld_post, nb,
                                           (unsigned char*)ws, s);
        }
        if (e == hipSuccess) return PL_OK;
        return hipfail(e, kFixed ? "fixed-point ldpc decode launch" : "layered ldpc decode launch");
    });
}

// Decode with an explicit workspace of ws_bytes (>= one unit when one is needed):
// the polar grid / LDPC chunk is clamped to what the workspace holds.
static int decode_impl(pl_plan* p, const double* llr, int64_t batch, int64_t ld, uint8_t* bits, int32_t* iters,
                       void* ws, size_t ws_bytes, hipStream_t s, bool zero_masks = false,
                       const DecodeDiag& dg = DecodeDiag()) {
    unsigned long long* const stamps = dg.stamps;
    if (p->layered) return lms_decode_impl<double>(p, llr, batch, ld, bits, iters, nullptr, 0, ws, ws_bytes, s);
    const size_t wmin = ws_min(p);
    if (wmin > 0 && (ws == nullptr || ws_bytes < wmin))
        return fail(PL_EINVAL, "workspace smaller than one unit (pl_plan_workspace_bytes)");
    if (p->kind == 0 && p->generic) {
        if (stamps) return fail(PL_EUNSUPPORTED, "stamps only for the tree kernel");
        // one workgroup per frame, masks = null: every frame
        hipError_t e = pl::nan_redo_launch(llr, ld, bits, batch, p->pg.N, p->pg.K, p->list_size, p->d_frozen_dec,
                                           p->d_info_pos, p->d_crc_g, nullptr, 0, 1, redo_metric(p),
                                           (unsigned char*)ws, ws_bytes, p->redo_blocks, s);
        return e == hipSuccess ? PL_OK : hipfail(e, "polar generic list launch");
    }
    if (p->kind == 0) {
        if (!p->tree && stamps) return fail(PL_EUNSUPPORTED, "stamps only for the tree kernel");
        const int64_t waves = (batch + p->fpw - 1) / p->fpw;
        // every wavefront of the decode resident at the small instance's occupancy:
        // that instance (not for the dead-store diagnostics, headline instance only)
        const bool small = p->tree_small && waves <= p->small_grid_max && dg.ds_mode == 0;
        const pl::TreeInfo& ti = small ? p->tinfo_small : p->tinfo;
        int64_t grid = std::min<int64_t>(waves, p->lane_grid_max);
        while (grid > 1 && polar_bytes(p, grid) > ws_bytes) grid = std::min<int64_t>(grid - 1, grid * ws_bytes / polar_bytes(p, grid));
        unsigned char* const base = (unsigned char*)ws;
        uint64_t* const masks = p->mask_bytes ? (uint64_t*)base : nullptr;
        unsigned char* const slices = base + p->head_bytes;  // the group counter: slices - kSchedBytes
        if (masks && zero_masks) {  // a caller-owned workspace: the masks may hold anything
            hipError_t e = hipMemsetAsync(masks, 0, (size_t)grid * 8 * pl::kNanMaskPasses, s);
            if (e != hipSuccess) return hipfail(e, "NaN mask reset");
        }
        // a list launch runs at most kNanMaskPasses passes of its grid (the masks' depth).  Three
        // steps per chunk, each with its own error, and a readback: a loop of its own, not for_chunks
        const int64_t step = masks ? grid * p->fpw * pl::kNanMaskPasses : batch;
        for (int64_t b0 = 0; b0 < batch; b0 += step) {
            const int64_t nb = std::min<int64_t>(step, batch - b0);
            const double* l0 = llr + b0 * ld;
            uint8_t* o0 = bits + b0 * p->pg.K;
            hipError_t e;
            if (p->tree)
                e = pl::tree_launch(ti, l0, ld, o0, p->d_frozen_dec, p->d_info_pos, nb, p->pg.K,
                                    p->sc ? 1 : p->list_size, slices, (int)grid, stamps, p->d_crc_g,
                                    p->sc ? (const void*)p->d_r0k : (const void*)masks, s, dg.ds_mode);
            else
                e = pl::lane_launch(p->lgeo, p->sc, l0, ld, o0, p->d_frozen_dec, p->d_info_pos, nb, slices, (int)grid,
                                    p->d_crc_g, masks, s);
            if (e != hipSuccess) return hipfail(e, "polar decode launch");
            if (masks && dg.flagged) {  // diagnostic: which frames of this pass group were flagged
                std::vector<uint64_t> mw((size_t)grid * pl::kNanMaskPasses);
                e = hipMemcpyAsync(mw.data(), masks, mw.size() * 8, hipMemcpyDeviceToHost, s);
                if (e == hipSuccess) e = hipStreamSynchronize(s);
                if (e != hipSuccess) return hipfail(e, "NaN mask readback");
                // word [w][ps] bit f = frame (ps * grid + w) * fpw + f (polar_tree.hip, polar_nan.hip)
                for (int64_t w = 0; w < grid; ++w)
                    for (int ps = 0; ps < pl::kNanMaskPasses; ++ps)
                        for (int f = 0; f < 64; ++f)
                            if ((mw[(size_t)w * pl::kNanMaskPasses + ps] >> f) & 1) {
                                const int64_t fr = ((int64_t)ps * grid + w) * p->fpw + f;
                                if (fr < nb) dg.flagged[b0 + fr] = 1;
                            }
            }
            if (masks) {
                // frames whose list saw a NaN metric, in the reference's candidate order
                e = pl::nan_redo_launch(l0, ld, o0, nb, p->pg.N, p->pg.K, p->list_size, p->d_frozen_dec,
                                        p->d_info_pos, p->d_crc_g, masks, (int)grid, p->fpw, redo_metric(p), slices,
                                        ws_bytes - p->head_bytes, p->redo_blocks, s);
                if (e != hipSuccess) return hipfail(e, "polar NaN redo launch");
            }
        }
        return PL_OK;
    }
    // Flooding LDPC, one workgroup per frame.  Messages in LDS: no workspace, and HIP caps a grid at
    // 2^32 work-items; messages in the workspace: chunks of the frames it holds.
    const int64_t step = p->lg.use_global ? std::min<int64_t>(p->ldpc_chunk, (int64_t)(ws_bytes / p->ws_unit))
                                          : kMaxLaunchItems / p->lg.threads;
    double* const work = p->lg.use_global ? (double*)ws : nullptr;
    return for_chunks(batch, step, [&](int64_t b0, int64_t nb) {
        const hipError_t e = pl::ldpc_launch(p->lg, p->ld, llr + b0 * ld, ld, bits + b0 * p->lg.n,
                                             iters ? iters + b0 : nullptr, nb, work, s);
        return e == hipSuccess ? PL_OK : hipfail(e, "ldpc decode launch");
    });
}

// The calling stream's workspace entry (created empty on first use).
static std::shared_ptr<Workspace> stream_entry(pl_plan* p, hipStream_t s) {
    std::lock_guard<std::mutex> lk(p->mu);
    std::shared_ptr<Workspace>& w = p->ws[s];
    if (!w) w = std::make_shared<Workspace>();
    return w;
}

// Grow `w` (its mutex held by the caller) to `need` bytes.  A buffer is only
// ever used by its own stream.  The new buffer is allocated while the old one
// is still held; only if the device is out of memory is the old one released
// (after draining its stream) before retrying, then halved down to one unit (the
// decode then runs fewer resident wavefronts / smaller chunks: decode_impl
// clamps to what the buffer holds).  A failure other than out-of-memory leaves
// the old buffer in place.  `retry`: also retry a request that fell back before.
static int grow_ws(pl_plan* p, Workspace* w, hipStream_t s, size_t need, bool retry) {
    if (w->bytes >= need) return PL_OK;
    if (!retry && w->ptr && w->failed_need && need <= w->failed_need) return PL_OK;  // fell back for this size
    const size_t unit = std::max<size_t>(ws_min(p), 1);
    size_t want = need;
    for (;;) {
        void* np = nullptr;
        hipError_t e = hipMalloc(&np, want);
        if (e == hipSuccess) {
            if (w->ptr) {
                // the old buffer may still be read by work queued on this stream
                const hipError_t se = w->drain(s);
                if (se != hipSuccess) {
                    hipFree(np);
                    return hipfail(se, "workspace regrow: stream synchronize");
                }
            }
            if (p->mask_bytes) {  // NaN masks start at zero (the decodes keep them so), before the buffer is published
                hipError_t me = hipMemsetAsync(np, 0, p->mask_bytes, s);
                if (me != hipSuccess) {
                    hipFree(np);  // the workspace stays empty: the next decode retries
                    return hipfail(me, "NaN mask reset");
                }
            }
            w->ptr = np;
            w->bytes = want;
            w->failed_need = want < need ? need : 0;
            return PL_OK;
        }
        (void)hipGetLastError();  // clear the sticky allocation error before retrying
        if (e != hipErrorOutOfMemory) return hipfail(e, "decode workspace");
        if (w->ptr) {  // make room: drain this stream, release its buffer, retry the same size
            const hipError_t se = w->drain(s);
            if (se != hipSuccess) return hipfail(se, "workspace regrow: stream synchronize");
            continue;
        }
        if (want <= unit) return hipfail(e, "decode workspace");
        want = std::max(unit, (want / 2) / unit * unit);
    }
}

// run(ws, bytes) on the calling stream's workspace, grown to `need` bytes (less after an
// out-of-memory fallback: `bytes` is what there is) and held locked for the whole call.
// need == 0: run(nullptr, 0) with no map entry made, so pl_plan_workspace_stats counts only
// streams that hold a buffer.  (A polar plan's need is never 0 for batch > 0 -- polar_bytes always
// includes a slice or redo_unit -- so its diagnostic decodes always take the entry, as they did
// when they took it unconditionally.)
template <class F>
static int with_stream_ws(pl_plan* p, hipStream_t s, size_t need, F&& run) {
    if (need == 0) return run(nullptr, (size_t)0);
    const std::shared_ptr<Workspace> w = stream_entry(p, s);
    std::lock_guard<std::mutex> lk(w->mu);
    if (const int rc = grow_ws(p, w.get(), s, need, false)) return rc;
    return run(w->ptr, (size_t)w->bytes);
}

// pl_decode and the diagnostic decodes: decode_impl on the calling stream's workspace
static int decode_on_stream(pl_plan* p, const double* llr, int64_t batch, int64_t ld, uint8_t* bits, int32_t* iters,
                            hipStream_t s, const DecodeDiag& dg = DecodeDiag()) {
    return with_stream_ws(p, s, ws_need(p, batch), [&](void* ws, size_t bytes) {
        return decode_impl(p, llr, batch, ld, bits, iters, ws, bytes, s, false, dg);
    });
}

static const char kFixedOnly[] =
    "a fixed-point plan (pl_ldpc_qc_fixed_plan_create) decodes int8 LLRs through pl_ldpc_decode_i8 only";

// i8: the call is pl_ldpc_decode_i8's; every floating-point entry point refuses a fixed-point plan
static int check_decode_args(const pl_plan* p, int64_t batch, int64_t ld, const void* llr, const void* bits,
                             bool i8 = false) {
    if (!p) return fail(PL_EINVAL, "plan is NULL");
    if (p->qc_fixed && !i8) return fail(PL_EUNSUPPORTED, kFixedOnly);
    if (batch < 0) return fail(PL_EINVAL, "batch < 0");
    if (batch > 0 && (!llr || !bits)) return fail(PL_EINVAL, "NULL buffer");
    if (p->kind == 0 && ld < p->pg.N) return fail(PL_EINVAL, "ld < N");
    if (p->kind == 1 && ld < p->lg.n) return fail(PL_EINVAL, "ld < n");
    if (p->kind == 0 && !p->decodable)
        return fail(PL_EUNSUPPORTED, "this plan's decoder needs more LDS than the device has (list_size 0 or 1 at "
                                     "N = 32768): it serves pl_polar_encode only");
    return PL_OK;
}

extern "C" int pl_plan_reserve(pl_plan* p, int64_t max_batch, void* stream) {
    if (!p) return fail(PL_EINVAL, "plan is NULL");
    if (max_batch < 0) return fail(PL_EINVAL, "max_batch < 0");
    if (max_batch == 0) return pl_plan_release(p, stream);
    int rc = check_device(p);
    if (rc) return rc;
    const size_t need = ws_need(p, max_batch);
    if (need == 0) return PL_OK;
    const hipStream_t s = (hipStream_t)stream;
    std::shared_ptr<Workspace> w = stream_entry(p, s);
    std::lock_guard<std::mutex> lk(w->mu);
    return grow_ws(p, w.get(), s, need, true);
}

extern "C" int pl_plan_release(pl_plan* p, void* stream) {
    if (!p) return fail(PL_EINVAL, "plan is NULL");
    if (int rc = check_device(p)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    std::shared_ptr<Workspace> w;
    {
        std::lock_guard<std::mutex> lk(p->mu);
        auto it = p->ws.find(s);
        if (it == p->ws.end()) return PL_OK;
        w = it->second;
        p->ws.erase(it);
    }
    std::lock_guard<std::mutex> lk(w->mu);  // a decode in flight on this stream finishes its launch first
    if (w->ptr) {
        const hipError_t e = w->drain(s);
        if (e != hipSuccess) return hipfail(e, "workspace release: stream synchronize");
    }
    return PL_OK;
}

extern "C" int pl_plan_workspace_stats(const pl_plan* p, int64_t* streams, int64_t* bytes) {
    if (!p || !streams || !bytes) return fail(PL_EINVAL, "NULL argument");
    std::lock_guard<std::mutex> lk(const_cast<pl_plan*>(p)->mu);
    *streams = 0;
    *bytes = 0;
    for (const auto& kv : p->ws) {
        ++*streams;
        *bytes += (int64_t)kv.second->bytes.load();
    }
    return PL_OK;
}

extern "C" int pl_plan_workspace_bytes(const pl_plan* p, int64_t batch, int64_t* bytes) {
    if (!p || !bytes) return fail(PL_EINVAL, "NULL argument");
    if (batch < 0) return fail(PL_EINVAL, "batch < 0");
    *bytes = (int64_t)ws_need(p, batch);
    return PL_OK;
}

extern "C" int pl_decode(pl_plan* p, const double* llr, int64_t batch, int64_t ld, uint8_t* bits,
                         int32_t* iters, void* stream) {
    int rc = check_decode_args(p, batch, ld, llr, bits);
    if (rc || batch == 0) return rc;
    if ((rc = check_device(p))) return rc;
    return decode_on_stream(p, llr, batch, ld, bits, iters, (hipStream_t)stream);
}

extern "C" int pl_decode_ws(pl_plan* p, const double* llr, int64_t batch, int64_t ld, uint8_t* bits,
                            int32_t* iters, void* workspace, int64_t workspace_bytes, void* stream) {
    int rc = check_decode_args(p, batch, ld, llr, bits);
    if (rc || batch == 0) return rc;
    if (workspace_bytes < 0) return fail(PL_EINVAL, "workspace_bytes < 0");
    if ((rc = check_device(p))) return rc;
    return decode_impl(p, llr, batch, ld, bits, iters, workspace, (size_t)workspace_bytes, (hipStream_t)stream,
                       true);
}

extern "C" int pl_ldpc_decode_soft(pl_plan* p, const double* llr, int64_t batch, int64_t ld, uint8_t* bits,
                                   int32_t* iters, double* post, int64_t ld_post, void* stream) {
    if (!p) return fail(PL_EINVAL, "plan is NULL");
    if (!p->layered) return fail(PL_EUNSUPPORTED, "posterior output: layered min-sum plans only");
    int rc = check_decode_args(p, batch, ld, llr, bits);
    if (rc) return rc;
    if (batch > 0 && !post) return fail(PL_EINVAL, "NULL buffer");
    if (ld_post < p->lms.n) return fail(PL_EINVAL, "ld_post < n");
    if (batch == 0) return PL_OK;
    if ((rc = check_device(p))) return rc;
    const hipStream_t s = (hipStream_t)stream;
    return with_stream_ws(p, s, ws_need(p, batch), [&](void* ws, size_t bytes) {
        return lms_decode_impl(p, llr, batch, ld, bits, iters, post, ld_post, ws, bytes, s);
    });
}

// pl_ldpc_decode_f32's and pl_ldpc_decode_i8's part behind their refusals by the plan's kind: on the
// caller's workspace, or with a null one on the stream's
template <typename IO>
static int lms_decode_typed(pl_plan* p, const IO* llr, int64_t batch, int64_t ld, uint8_t* bits, int32_t* iters,
                            IO* post, int64_t ld_post, void* workspace, int64_t workspace_bytes, hipStream_t s) {
    int rc = check_decode_args(p, batch, ld, llr, bits, std::is_same<IO, int8_t>::value);
    if (rc) return rc;
    if (post && ld_post < p->lms.n) return fail(PL_EINVAL, "ld_post < n");
    if (workspace && workspace_bytes < 0) return fail(PL_EINVAL, "workspace_bytes < 0");
    if (batch == 0) return PL_OK;
    if ((rc = check_device(p))) return rc;
    if (workspace)
        return lms_decode_impl(p, llr, batch, ld, bits, iters, post, ld_post, workspace, (size_t)workspace_bytes, s);
    return with_stream_ws(p, s, ws_need(p, batch), [&](void* ws, size_t bytes) {
        return lms_decode_impl(p, llr, batch, ld, bits, iters, post, ld_post, ws, bytes, s);
    });
}

extern "C" int pl_ldpc_decode_f32(pl_plan* p, const float* llr, int64_t batch, int64_t ld, uint8_t* bits,
                                  int32_t* iters, float* post, int64_t ld_post, void* workspace,
                                  int64_t workspace_bytes, void* stream) {
    if (!p) return fail(PL_EINVAL, "plan is NULL");
    if (p->qc_fixed) return fail(PL_EUNSUPPORTED, kFixedOnly);
    if (!p->qc || !p->qc_f32)
        return fail(PL_EUNSUPPORTED, "fp32 LLRs: quasi-cyclic plans created with PL_LDPC_QC_F32 only");
    return lms_decode_typed(p, llr, batch, ld, bits, iters, post, ld_post, workspace, workspace_bytes,
                            (hipStream_t)stream);
}

extern "C" int pl_ldpc_decode_i8(pl_plan* p, const int8_t* llr, int64_t batch, int64_t ld, uint8_t* bits,
                                 int32_t* iters, int8_t* post, int64_t ld_post, void* workspace,
                                 int64_t workspace_bytes, void* stream) {
    if (!p) return fail(PL_EINVAL, "plan is NULL");
    if (!p->qc_fixed)
        return fail(PL_EUNSUPPORTED, "int8 LLRs: fixed-point plans (pl_ldpc_qc_fixed_plan_create) only");
    return lms_decode_typed(p, llr, batch, ld, bits, iters, post, ld_post, workspace, workspace_bytes,
                            (hipStream_t)stream);
}

extern "C" int pl_llr_quantize(const void* llr, int32_t flags, int64_t ld, int64_t batch, int32_t n, double scale,
                               int32_t llr_max, int8_t* out, int64_t ld_out, void* stream) {
    if (flags & ~PL_QUANT_LLR_F32) return fail(PL_EINVAL, "unknown flag bits");
    if (batch < 0) return fail(PL_EINVAL, "batch must be >= 0");
    if (n < 1) return fail(PL_EINVAL, "n must be >= 1");
    if (!(scale > 0.0) || !std::isfinite(scale)) return fail(PL_EINVAL, "scale must be finite and > 0");
    if (llr_max < 1 || llr_max > 127) return fail(PL_EINVAL, "llr_max = " + std::to_string(llr_max) + " outside 1 .. 127");
    if (ld < n) return fail(PL_EINVAL, "ld < n");
    if (ld_out < n) return fail(PL_EINVAL, "ld_out < n");
    if (batch == 0) return PL_OK;
    if (!llr || !out) return fail(PL_EINVAL, "device pointers must not be NULL");
    if ((uintptr_t)llr & ((flags & PL_QUANT_LLR_F32) ? 3 : 7))
        return fail(PL_EINVAL, "llr_dev must be aligned to its element type");
    const hipError_t e = pl::llr_quantize_launch(llr, flags & PL_QUANT_LLR_F32, ld, batch, n, scale, llr_max, out,
                                                 ld_out, (hipStream_t)stream);
    return e == hipSuccess ? PL_OK : hipfail(e, "llr quantize launch");
}

extern "C" int pl_debug_polar_stamps(pl_plan* p, const double* llr, int64_t batch, int64_t ld, uint8_t* bits,
                                     unsigned long long* stamps_dev, void* stream) {
    if (!p || p->kind != 0 || !stamps_dev) return fail(PL_EINVAL, "polar plan and stamp buffer required");
#if !PL_DIAG
    (void)llr; (void)batch; (void)ld; (void)bits; (void)stream;
    return fail(PL_EUNSUPPORTED, "stamped kernels are in the diagnostic build only (make DIAG=1)");
#else
    int rc = check_decode_args(p, batch, ld, llr, bits);
    if (rc || batch == 0) return rc;
    if ((rc = check_device(p))) return rc;
    DecodeDiag dg;
    dg.stamps = stamps_dev;
    return decode_on_stream(p, llr, batch, ld, bits, nullptr, (hipStream_t)stream, dg);
#endif
}

extern "C" int pl_debug_polar_deadstore(pl_plan* p, const double* llr, int64_t batch, int64_t ld, uint8_t* bits,
                                        uint32_t* mask_dev, int32_t mode, void* stream) {
    if (!p || p->kind != 0 || !mask_dev || (mode != 1 && mode != 2)) return fail(PL_EINVAL, "polar plan, mask, mode 1|2");
#if !PL_DIAG
    (void)llr; (void)batch; (void)ld; (void)bits; (void)stream;
    return fail(PL_EUNSUPPORTED, "dead-store instances are in the diagnostic build only (make DIAG=1)");
#else
    int rc = check_decode_args(p, batch, ld, llr, bits);
    if (rc || batch == 0) return rc;
    if ((rc = check_device(p))) return rc;
    if (!p->tree || !p->tinfo.fn_ds[0]) return fail(PL_EUNSUPPORTED, "dead-store instances: N=1024 L=8 tree plans only");
    DecodeDiag dg;
    dg.stamps = reinterpret_cast<unsigned long long*>(mask_dev);
    dg.ds_mode = mode;
    return decode_on_stream(p, llr, batch, ld, bits, nullptr, (hipStream_t)stream, dg);
#endif
}

// Diagnostic build: an ordinary list decode that also reports, per frame, whether
// the list kernel flagged it for the NaN-order redo decoder (flagged_host: `batch`
// bytes, 1 = flagged).  The decode itself is the product path, bits included.
extern "C" int pl_debug_polar_flagged(pl_plan* p, const double* llr, int64_t batch, int64_t ld, uint8_t* bits,
                                      uint8_t* flagged_host, void* stream) {
    if (!p || p->kind != 0 || !flagged_host) return fail(PL_EINVAL, "polar plan and flag array required");
#if !PL_DIAG
    (void)llr; (void)batch; (void)ld; (void)bits; (void)stream;
    return fail(PL_EUNSUPPORTED, "test hook: diagnostic build only (make DIAG=1)");
#else
    int rc = check_decode_args(p, batch, ld, llr, bits);
    if (rc || batch == 0) return rc;
    if ((rc = check_device(p))) return rc;
    if (p->generic || p->mask_bytes == 0) return fail(PL_EUNSUPPORTED, "plan has no NaN masks (SC or generic list plan)");
    std::memset(flagged_host, 0, (size_t)batch);
    DecodeDiag dg;
    dg.flagged = flagged_host;
    return decode_on_stream(p, llr, batch, ld, bits, nullptr, (hipStream_t)stream, dg);
#endif
}

extern "C" int pl_debug_ldpc_stamps(pl_plan* p, const double* llr, int64_t batch, int64_t ld, uint8_t* bits,
                                    int32_t* iters, unsigned long long* stamps_dev, void* stream) {
    if (!p || p->kind != 1 || !stamps_dev) return fail(PL_EINVAL, "LDPC plan and stamp buffer required");
#if !PL_DIAG
    (void)llr; (void)batch; (void)ld; (void)bits; (void)iters; (void)stream;
    return fail(PL_EUNSUPPORTED, "stamped kernels are in the diagnostic build only (make DIAG=1)");
#else
    int rc = check_decode_args(p, batch, ld, llr, bits);
    if (rc || batch == 0) return rc;
    if ((rc = check_device(p))) return rc;
    if (!p->lg.grp || p->lg.reg_variant != 1) return fail(PL_EUNSUPPORTED, "stamps only for the grouped (504,252)-size BP kernel");
    hipError_t e = pl::ldpc_launch_stamped(p->lg, p->ld, llr, ld, bits, iters, batch, stamps_dev, (hipStream_t)stream);
    return e == hipSuccess ? PL_OK : hipfail(e, "stamped LDPC launch");
#endif
}

// Diagnostic build: the frame-per-wavefront prototype (polar_fpw.hip) on a
// polar N=1024 L=8 plan's device constants; stamps_dev: 5 u64 cycle sums
// (descent, metric, prune, partial sums, output); grid 0 = fill the device.
extern "C" int pl_debug_polar_fpw(pl_plan* p, const double* llr, int64_t batch, int64_t ld, uint8_t* bits,
                                  unsigned long long* stamps_dev, int32_t grid, void* stream) {
#if !PL_DIAG
    (void)p; (void)llr; (void)batch; (void)ld; (void)bits; (void)stamps_dev; (void)grid; (void)stream;
    return fail(PL_EUNSUPPORTED, "the frame-per-wavefront prototype is in the diagnostic build only (make DIAG=1)");
#else
    if (!p || p->kind != 0 || p->pg.N != 1024 || p->list_size != 8) return fail(PL_EINVAL, "N=1024 L=8 polar plan");
    int rc = check_decode_args(p, batch, ld, llr, bits);
    if (rc || batch == 0) return rc;
    if ((rc = check_device(p))) return rc;
    hipError_t e = pl::fpw_launch(llr, ld, bits, p->d_frozen_dec, p->d_info_pos, batch, p->pg.K, stamps_dev, grid,
                                  (hipStream_t)stream);
    return e == hipSuccess ? PL_OK : hipfail(e, "fpw launch");
#endif
}

extern "C" int pl_debug_set_plan_device(pl_plan* p, int32_t device) {
    if (!p) return fail(PL_EINVAL, "plan is NULL");
#if !PL_DIAG
    (void)device;
    return fail(PL_EUNSUPPORTED, "test hook: diagnostic build only (make DIAG=1)");
#else
    p->device = device;
    return PL_OK;
#endif
}

extern "C" int pl_polar_plan_set_crc(pl_plan* p, int32_t crc_len, uint32_t poly) {
    if (!p || p->kind != 0) return fail(PL_EINVAL, "not a polar plan");
    if (p->sc) return fail(PL_EINVAL, "CRC-aided selection needs a list decoder (list_size >= 1)");
    if (crc_len < 0 || crc_len > 32) return fail(PL_EINVAL, "crc_len must be in [0, 32]");
    if (int rc = check_device(p)) return rc;
    if (p->d_crc_g) { hipFree(p->d_crc_g); p->d_crc_g = nullptr; }
    if (crc_len == 0) return PL_OK;
    const int N = p->pg.N;
    // g[j] = CRC register (src/polar/utils.py:86-125, zero initial register) of
    // the info bits of u = e_j F^{(x)n}; u_k = 1 iff k is a bit-submask of j.
    const uint32_t top = 1u << (crc_len - 1), mask = crc_len == 32 ? 0xFFFFFFFFu : ((1u << crc_len) - 1u);
    std::vector<uint32_t> g((size_t)N);
    for (int j = 0; j < N; ++j) {
        uint32_t crc = 0;
        for (const int32_t k : p->h_info) {
            const uint32_t bit = ((k & j) == k) ? 1u : 0u;
            crc ^= bit << (crc_len - 1);
            crc = (crc & top) ? ((crc << 1) ^ poly) : (crc << 1);
            crc &= mask;
        }
        g[(size_t)j] = crc;
    }
    hipError_t e = upload(&p->d_crc_g, g);
    return e == hipSuccess ? PL_OK : hipfail(e, "crc table upload");
}

extern "C" int pl_plan_get_info(const pl_plan* p, pl_plan_info* info) {
    if (!p || !info) return fail(PL_EINVAL, "NULL argument");
    *info = pl_plan_info{};
    if (p->kind == 0) {
        info->kind = 0; info->n_in = p->pg.N; info->n_out = p->pg.K; info->list_size = p->list_size;
        info->lds_bytes = p->pg.lds_bytes; info->fused_top = p->pg.F;
        info->frames_per_block = p->fpw;
        info->reserved = p->generic ? 6 : (p->tree ? 4 : 3);  // kernel: 4 tree, 3 lane, 6 single-workgroup exact
    } else if (p->layered) {
        info->kind = 1; info->n_in = p->lms.n; info->n_out = p->lms.n; info->list_size = 0;
        info->lds_bytes = p->lms.lds_bytes; info->fused_top = 0; info->frames_per_block = p->lms.fpb;
        info->reserved = pl::lms_kernel_code(p->lms);  // layered min-sum: 9 state in LDS, 10 in the workspace
        if (p->qc_bp) {
            info->lds_bytes = p->qbg.lds_bytes; info->frames_per_block = p->qbg.fpw * p->qbg.fpb;
            info->reserved = pl::qc_bp_kernel_code(p->qbg);  // quasi-cyclic sum-product: 17 in LDS, 18 in the workspace
        } else if (p->qc || p->qc_fixed) {
            const pl::QcMap& q = p->qc ? static_cast<const pl::QcMap&>(p->qcg) : p->qfg;
            info->lds_bytes = q.lds_bytes; info->frames_per_block = q.fpw * q.fpb;
            // quasi-cyclic layered min-sum: 11 state in LDS, 12 in the workspace; fp32 state: 13, 14; int8
            // fixed point: 15, 16
            info->reserved = p->qc ? pl::qc_kernel_code(p->qcg, p->qc_f32) : pl::qc_fixed_kernel_code(p->qfg);
            // the fixed-point instance: inputs of a check kept in registers, 0 the two-pass form
            if (p->qc_fixed) info->fused_top = q.dcap;
        }
    } else {
        info->kind = 1; info->n_in = p->lg.n; info->n_out = p->lg.n; info->list_size = 0;
        info->lds_bytes = p->lg.lds_bytes; info->fused_top = 0; info->frames_per_block = p->lg.fpg > 1 ? p->lg.fpg : 1;
        // kernel: 2 register-cached, 7 register-cached BP with degree-grouped products,
        // 1 generic (LDS or global workspace), 3 thread-per-check, 5 min-sum with compressed check state,
        // 8 (3,6)-regular min-sum with rebuild-ready check state
        info->reserved = pl::ldpc_kernel_code(p->lg);
    }
    return PL_OK;
}

extern "C" int pl_polar_plan_small_batch(const pl_plan* p, int64_t* max_frames) {
    if (!p || !max_frames) return fail(PL_EINVAL, "NULL argument");
    *max_frames = (p->kind == 0 && p->tree_small) ? (int64_t)p->small_grid_max * p->fpw : 0;
    return PL_OK;
}

extern "C" int pl_plan_destroy(pl_plan* p) {
    if (!p) return PL_OK;
    if (p->d_frozen_dec) hipFree(p->d_frozen_dec);
    if (p->d_info_pos) hipFree(p->d_info_pos);
    if (p->d_crc_g) hipFree(p->d_crc_g);
    if (p->d_r0k) hipFree(p->d_r0k);
    if (p->d_ldpc) hipFree(p->d_ldpc);
    p->ws.clear();  // each Workspace frees its buffer (hipFree waits for work that still uses it)
    delete p;
    return PL_OK;
}

extern "C" int pl_random_bits(uint64_t seed, int64_t frame_offset, int64_t batch, int32_t k, uint8_t* bits,
                              void* stream) {
    if (batch < 0 || k < 0 || (!bits && batch * k > 0)) return fail(PL_EINVAL, "bad argument");
    hipError_t e = pl::random_bits_launch(seed, frame_offset, batch, k, bits, (hipStream_t)stream);
    return e == hipSuccess ? PL_OK : hipfail(e, "random bits launch");
}

extern "C" int pl_polar_encode(const pl_plan* p, const uint8_t* msg, int64_t batch, uint8_t* cw, void* stream) {
    if (!p || p->kind != 0) return fail(PL_EINVAL, "not a polar plan");
    if (batch < 0 || (batch > 0 && (!msg || !cw))) return fail(PL_EINVAL, "bad argument");
    if (int rc = check_device(p)) return rc;
    const int64_t step = kMaxLaunchItems / 64;  // one wavefront per frame
    return for_chunks(batch, step, [&](int64_t b0, int64_t nb) {
        const hipError_t e = pl::polar_encode_launch(p->pg.N, p->pg.K, p->d_info_pos, msg + b0 * p->pg.K, nb,
                                                     cw + b0 * p->pg.N, (hipStream_t)stream);
        return e == hipSuccess ? PL_OK : hipfail(e, "polar encode launch");
    });
}

extern "C" int pl_awgn_llr(const uint8_t* cw, int32_t n, int64_t batch, double snr_db, uint64_t seed,
                           int64_t frame_offset, double* llr, int64_t ld, void* stream) {
    if (n < 1 || batch < 0 || ld < n || (!llr && batch > 0)) return fail(PL_EINVAL, "bad argument");
    // src/channel/awgn.py:27-32 -- same double-precision expression order
    const double snr_linear = std::pow(10.0, snr_db / 10.0);
    const double sigma = std::sqrt(1.0 / (2.0 * snr_linear));
    const double sigma2 = sigma * sigma;
    hipError_t e = pl::awgn_launch(cw, n, batch, sigma, sigma2, seed, frame_offset, llr, ld, (hipStream_t)stream);
    return e == hipSuccess ? PL_OK : hipfail(e, "awgn launch");
}

extern "C" int pl_rayleigh_llr(const uint8_t* cw, int32_t n, int64_t batch, double snr_db, uint64_t seed,
                               int64_t frame_offset, double* llr, int64_t ld, void* stream) {
    if (n < 1 || batch < 0 || ld < n || (!llr && batch > 0)) return fail(PL_EINVAL, "bad argument");
    const double snr_linear = std::pow(10.0, snr_db / 10.0);  // src/channel/fading.py:21-23
    const double sigma = std::sqrt(1.0 / (2.0 * snr_linear));
    hipError_t e = pl::rayleigh_launch(cw, n, batch, sigma, sigma * sigma, seed, frame_offset, llr, ld,
                                       (hipStream_t)stream);
    return e == hipSuccess ? PL_OK : hipfail(e, "rayleigh launch");
}

extern "C" int pl_bsc(const uint8_t* cw, int32_t n, int64_t batch, double crossover_prob, uint64_t seed,
                      int64_t frame_offset, uint8_t* out, int64_t ld, void* stream) {
    if (n < 1 || batch < 0 || ld < n || !(crossover_prob >= 0.0 && crossover_prob <= 1.0) || (!out && batch > 0))
        return fail(PL_EINVAL, "bad argument (crossover probability must be in [0, 1])");  // bsc.py:26
    hipError_t e = pl::bsc_launch(cw, n, batch, crossover_prob, seed, frame_offset, out, ld, (hipStream_t)stream);
    return e == hipSuccess ? PL_OK : hipfail(e, "bsc launch");
}

extern "C" int pl_crc_append(uint8_t* msg, int64_t ld, int64_t batch, int32_t k_data, int32_t crc_len,
                             uint32_t poly, void* stream) {
    if (batch < 0 || k_data < 0 || crc_len < 1 || crc_len > 32 || ld < (int64_t)k_data + crc_len ||
        (batch > 0 && !msg))
        return fail(PL_EINVAL, "bad argument");
    hipError_t e = pl::crc_append_launch(msg, ld, batch, k_data, crc_len, poly, (hipStream_t)stream);
    return e == hipSuccess ? PL_OK : hipfail(e, "crc append launch");
}

extern "C" int pl_gf2_encode(const uint32_t* g_dev, int32_t k, int32_t n, const uint8_t* msg, int64_t ld_msg,
                             int64_t batch, uint8_t* cw, int64_t ld_cw, void* stream) {
    if (batch < 0 || k < 1 || n < 1 || ld_msg < k || ld_cw < n || (batch > 0 && (!g_dev || !msg || !cw)))
        return fail(PL_EINVAL, "bad argument");
    const int64_t step = kMaxLaunchItems / 64;  // one wavefront per frame
    return for_chunks(batch, step, [&](int64_t b0, int64_t nb) {
        const hipError_t e = pl::gf2_encode_launch(g_dev, k, n, msg + b0 * ld_msg, ld_msg, nb, cw + b0 * ld_cw, ld_cw,
                                                   (hipStream_t)stream);
        return e == hipSuccess ? PL_OK : hipfail(e, "gf2 encode launch");
    });
}

// ---- quasi-cyclic encoder from the base matrix (ldpc_qc_encode.hip) ----
struct pl_qc_encoder {
    int device = 0;
    pl::QcEncGeom g{};
    int32_t* d_tab = nullptr;  // the planner's stream
};

extern "C" int pl_ldpc_qc_encoder_create(int32_t mb, int32_t nb, int32_t z, const int32_t* shift,
                                         pl_qc_encoder** out) {
    if (!out) return fail(PL_EINVAL, "out is NULL");
    *out = nullptr;
    // every argument check (ldpc_plan.cpp) comes before the first device call
    pl::QcEncHostPlan hp;
    const pl::PlanStatus st = pl::qc_encoder_plan_build(mb, nb, z, shift, &hp);
    if (st.code) return fail(st.code, st.msg);
    int dev = -1;
    const hipError_t ge = hipGetDevice(&dev);
    if (ge != hipSuccess) return hipfail(ge, "hipGetDevice");
    std::unique_ptr<pl_qc_encoder, Destroyer<pl_qc_encoder, pl_ldpc_qc_encoder_destroy>> e(new pl_qc_encoder());
    e->g = hp.geom;
    e->device = dev;
    hipError_t err = upload(&e->d_tab, hp.tables);
    if (err == hipSuccess) err = pl::qc_encode_prepare(e->g);
    if (err != hipSuccess) return hipfail(err, "encoder upload");
    *out = e.release();
    return PL_OK;
}

extern "C" int pl_ldpc_qc_encode(const pl_qc_encoder* enc, const uint8_t* msg, int64_t ld_msg, int64_t batch,
                                 uint8_t* cw, int64_t ld_cw, void* stream) {
    if (!enc) return fail(PL_EINVAL, "encoder is NULL");
    if (!msg || !cw) return fail(PL_EINVAL, "msg_dev and cw_dev must not be NULL");
    if (batch < 0) return fail(PL_EINVAL, "batch must be >= 0");
    if (ld_msg < enc->g.k) return fail(PL_EINVAL, "ld_msg < k = " + std::to_string(enc->g.k));
    if (ld_cw < enc->g.n) return fail(PL_EINVAL, "ld_cw < n = " + std::to_string(enc->g.n));
    if (int rc = check_device(enc->device, "encoder's")) return rc;
    // whole workgroups per launch, below kMaxLaunchItems work-items
    const int64_t step = kMaxLaunchItems / enc->g.threads * ((int64_t)enc->g.fpw * enc->g.fpb);
    return for_chunks(batch, step, [&](int64_t b0, int64_t nb) {
        const hipError_t e = pl::qc_encode_launch(enc->g, enc->d_tab, msg + b0 * ld_msg, ld_msg, nb, cw + b0 * ld_cw,
                                                  ld_cw, (hipStream_t)stream);
        return e == hipSuccess ? PL_OK : hipfail(e, "qc encode launch");
    });
}

extern "C" int pl_ldpc_qc_encoder_destroy(pl_qc_encoder* enc) {
    if (!enc) return PL_OK;
    if (enc->d_tab) hipFree(enc->d_tab);
    delete enc;
    return PL_OK;
}

// The planner's decisions for an encoder, with no device call.
extern "C" int pl_debug_ldpc_qc_encoder_probe(int32_t mb, int32_t nb, int32_t z, const int32_t* shift,
                                              pl_qc_encoder_probe* out) {
    if (!out) return fail(PL_EINVAL, "out is NULL");
    pl::QcEncHostPlan hp;
    const pl::PlanStatus st = pl::qc_encoder_plan_build(mb, nb, z, shift, &hp);
    if (st.code) return fail(st.code, st.msg);
    const pl::QcEncGeom& g = hp.geom;
    *out = pl_qc_encoder_probe{g.g, hp.x, hp.a, hp.b, g.subwave, g.fpw, g.fpb, g.threads, g.lds_bytes, hp.n_sync,
                               (int64_t)hp.tables.size(), pl::plan_tables_digest(hp.tables)};
    return PL_OK;
}

extern "C" int pl_debug_set_qc_encoder_device(pl_qc_encoder* enc, int32_t device) {
    if (!enc) return fail(PL_EINVAL, "encoder is NULL");
#if !PL_DIAG
    (void)device;
    return fail(PL_EUNSUPPORTED, "test hook: diagnostic build only (make DIAG=1)");
#else
    enc->device = device;
    return PL_OK;
#endif
}

// ---- rate matching of quasi-cyclic codes (ldpc_qc_ratematch.hip) ----
extern "C" int pl_ldpc_rate_match_check(pl_rate_match* rm) {
    const pl::PlanStatus st = pl::rate_match_check(rm);
    return st.code ? fail(st.code, st.msg) : PL_OK;
}

extern "C" int pl_debug_rate_match_probe(int32_t mb, int32_t nb, int32_t z, int32_t punctured, int32_t fillers,
                                         int32_t ncb, int32_t start, int32_t E, pl_rate_match* out) {
    if (!out) return fail(PL_EINVAL, "out is NULL");
    pl_rate_match rm{};
    rm.mb = mb; rm.nb = nb; rm.z = z;
    rm.punctured = punctured; rm.fillers = fillers; rm.ncb = ncb; rm.start = start; rm.E = E;
    if (int rc = pl_ldpc_rate_match_check(&rm)) return rc;
    *out = rm;
    return PL_OK;
}

// the caller's parameters, checked and derived afresh; every check comes before the first device call
static int rate_match_args(const pl_rate_match* in, pl_rate_match* rm, const void* a, const void* b, int64_t batch) {
    if (!in) return fail(PL_EINVAL, "rate match is NULL");
    *rm = *in;
    if (int rc = pl_ldpc_rate_match_check(rm)) return rc;
    if (!a || !b) return fail(PL_EINVAL, "device pointers must not be NULL");
    if (batch < 0) return fail(PL_EINVAL, "batch must be >= 0");
    return PL_OK;
}

extern "C" int pl_ldpc_rate_match(const pl_rate_match* in, const uint8_t* cw, int64_t ld_cw, int64_t batch, uint8_t* e,
                                  int64_t ld_e, void* stream) {
    pl_rate_match rm;
    if (int rc = rate_match_args(in, &rm, cw, e, batch)) return rc;
    if (ld_cw < rm.n) return fail(PL_EINVAL, "ld_cw < n = " + std::to_string(rm.n));
    if (ld_e < rm.E) return fail(PL_EINVAL, "ld_e < E = " + std::to_string(rm.E));
    const hipError_t err = pl::rate_match_launch(rm, cw, ld_cw, batch, e, ld_e, (hipStream_t)stream);
    return err == hipSuccess ? PL_OK : hipfail(err, "rate match launch");
}

extern "C" int pl_ldpc_rate_recover(const pl_rate_match* in, const void* llr, int64_t ld_llr, int64_t batch, void* out,
                                    int64_t ld_out, int32_t n_out, double filler_llr, int32_t flags, void* stream) {
    pl_rate_match rm;
    if (int rc = rate_match_args(in, &rm, llr, out, batch)) return rc;
    if (flags & ~(PL_RM_LLR_F32 | PL_RM_OUT_F32 | PL_RM_ACCUMULATE)) return fail(PL_EINVAL, "unknown flag bits");
    if (n_out <= rm.hi)
        return fail(PL_EINVAL, "n_out = " + std::to_string(n_out) + " does not reach the highest transmitted position " +
                                   std::to_string(rm.hi));
    if (n_out > rm.n) return fail(PL_EINVAL, "n_out = " + std::to_string(n_out) + " > n = " + std::to_string(rm.n));
    if (((uintptr_t)llr & ((flags & PL_RM_LLR_F32) ? 3 : 7)) || ((uintptr_t)out & ((flags & PL_RM_OUT_F32) ? 3 : 7)))
        return fail(PL_EINVAL, "llr_dev and out_dev must be aligned to their element type");
    if (ld_llr < rm.E) return fail(PL_EINVAL, "ld_llr < E = " + std::to_string(rm.E));
    if (ld_out < n_out) return fail(PL_EINVAL, "ld_out < n_out = " + std::to_string(n_out));
    const hipError_t err = pl::rate_recover_launch(rm, llr, ld_llr, flags & PL_RM_LLR_F32, batch, out, ld_out,
                                                   flags & PL_RM_OUT_F32, n_out, filler_llr,
                                                   flags & PL_RM_ACCUMULATE, (hipStream_t)stream);
    return err == hipSuccess ? PL_OK : hipfail(err, "rate recover launch");
}

// ---- rate matching of polar codes (polar_ratematch.hip); the definition: include/polarldpc.h, pl_polar_rm ----
extern "C" int pl_polar_rate_match_check(pl_polar_rm* rm) {
    if (!rm) return fail(PL_EINVAL, "rate match is NULL");
    const auto S = [](int64_t v) { return std::to_string(v); };
    const int64_t N = rm->N, E = rm->E, nsub = rm->nsub;
    if (N < 2 || N > 32768 || (N & (N - 1))) return fail(PL_EINVAL, "N = " + S(N) + " must be a power of 2 in 2 .. 32768");
    if (E < 1 || E > ((int64_t)1 << 30)) return fail(PL_EINVAL, "E = " + S(E) + " outside 1 .. 2^30");
    if (rm->mode != PL_PRM_PUNCTURE && rm->mode != PL_PRM_SHORTEN)
        return fail(PL_EINVAL, "mode = " + S(rm->mode) + " must be PL_PRM_PUNCTURE (0) or PL_PRM_SHORTEN (1)");
    if (nsub < 1 || nsub > 32 || (nsub & (nsub - 1)) || nsub > N)
        return fail(PL_EINVAL, "nsub = " + S(nsub) + " must be a power of 2 in 1 .. 32 and <= N = " + S(N));
    uint8_t inv[32] = {};
    uint32_t seen = 0;
    for (int64_t q = 0; q < nsub; ++q) {
        const uint32_t v = rm->perm[q];
        if (v >= nsub || (seen >> v & 1u))
            return fail(PL_EINVAL, "perm[0:nsub] is no permutation of 0 .. nsub-1 = " + S(nsub - 1) + " (perm[" + S(q) +
                                       "] = " + S(v) + ")");
        seen |= 1u << v;
        inv[v] = (uint8_t)q;
    }
    rm->S = (int32_t)(N / nsub);
    rm->U = (int32_t)(E < N ? N - E : 0);
    rm->max_reps = (int32_t)((E + N - 1) / N);
    rm->pad = 0;
    std::memcpy(rm->inv, inv, sizeof inv);
    return PL_OK;
}

extern "C" int pl_debug_polar_rate_match_probe(int32_t N, int32_t E, int32_t mode, int32_t nsub, const uint8_t* perm,
                                               pl_polar_rm* out) {
    if (!out) return fail(PL_EINVAL, "out is NULL");
    pl_polar_rm rm{};
    rm.N = N; rm.E = E; rm.mode = mode; rm.nsub = nsub;
    if (perm && nsub >= 1 && nsub <= 32) std::memcpy(rm.perm, perm, (size_t)nsub);
    if (int rc = pl_polar_rate_match_check(&rm)) return rc;
    *out = rm;
    return PL_OK;
}

extern "C" int pl_polar_rate_match_forced(const pl_polar_rm* in, uint8_t* mask) {
    if (!in) return fail(PL_EINVAL, "rate match is NULL");
    pl_polar_rm rm = *in;
    if (int rc = pl_polar_rate_match_check(&rm)) return rc;
    if (!mask) return fail(PL_EINVAL, "mask_host is NULL");
    std::memset(mask, 0, (size_t)rm.N);
    if (rm.mode != PL_PRM_SHORTEN || rm.E >= rm.N) return PL_OK;
    for (int32_t m = rm.E; m < rm.N; ++m) mask[rm.perm[m / rm.S] * rm.S + m % rm.S] = 1;  // x_J(m) is not sent
    // OR over subsets: afterwards mask[j] = 1 iff j is a superset of a position that is not sent
    for (int32_t b = 1; b < rm.N; b <<= 1)
        for (int32_t j = 0; j < rm.N; ++j)
            if (j & b) mask[j] |= mask[j ^ b];
    return PL_OK;
}

// the caller's parameters, checked and derived afresh; every check comes before the first device call
static int polar_rate_match_args(const pl_polar_rm* in, pl_polar_rm* rm, const void* a, const void* b, int64_t batch) {
    if (!in) return fail(PL_EINVAL, "rate match is NULL");
    *rm = *in;
    if (int rc = pl_polar_rate_match_check(rm)) return rc;
    if (!a || !b) return fail(PL_EINVAL, "device pointers must not be NULL");
    if (batch < 0) return fail(PL_EINVAL, "batch must be >= 0");
    return PL_OK;
}

extern "C" int pl_polar_rate_match(const pl_polar_rm* in, const uint8_t* cw, int64_t ld_cw, int64_t batch, uint8_t* e,
                                   int64_t ld_e, void* stream) {
    pl_polar_rm rm;
    if (int rc = polar_rate_match_args(in, &rm, cw, e, batch)) return rc;
    if (ld_cw < rm.N) return fail(PL_EINVAL, "ld_cw < N = " + std::to_string(rm.N));
    if (ld_e < rm.E) return fail(PL_EINVAL, "ld_e < E = " + std::to_string(rm.E));
    const hipError_t err = pl::polar_rate_match_launch(rm, cw, ld_cw, batch, e, ld_e, (hipStream_t)stream);
    return err == hipSuccess ? PL_OK : hipfail(err, "polar rate match launch");
}

extern "C" int pl_polar_rate_recover(const pl_polar_rm* in, const void* llr, int64_t ld_llr, int64_t batch, double* out,
                                     int64_t ld_out, double known_llr, int32_t flags, void* stream) {
    pl_polar_rm rm;
    if (int rc = polar_rate_match_args(in, &rm, llr, out, batch)) return rc;
    if (flags & ~(PL_PRM_LLR_F32 | PL_PRM_ACCUMULATE)) return fail(PL_EINVAL, "unknown flag bits");
    if (!(known_llr > 0.0) || !std::isfinite(known_llr)) return fail(PL_EINVAL, "known_llr must be finite and > 0");
    if (((uintptr_t)llr & ((flags & PL_PRM_LLR_F32) ? 3 : 7)) || ((uintptr_t)out & 7))
        return fail(PL_EINVAL, "llr_dev and out_dev must be aligned to their element type");
    if (ld_llr < rm.E) return fail(PL_EINVAL, "ld_llr < E = " + std::to_string(rm.E));
    if (ld_out < rm.N) return fail(PL_EINVAL, "ld_out < N = " + std::to_string(rm.N));
    const hipError_t err = pl::polar_rate_recover_launch(rm, llr, ld_llr, flags & PL_PRM_LLR_F32, batch, out, ld_out,
                                                         known_llr, flags & PL_PRM_ACCUMULATE, (hipStream_t)stream);
    return err == hipSuccess ? PL_OK : hipfail(err, "polar rate recover launch");
}

// ---- Gray-mapped QAM (qam.hip); the definition: include/polarldpc.h, pl_qam_check ----
extern "C" int pl_qam_check(int32_t m, int64_t E, int64_t* S, double* scale) {
    const pl::QamStatus st = pl::qam_check(m, E, S, scale);
    return st.code ? fail(st.code, st.msg) : PL_OK;
}

// what the three entry points share, every check before the first device call
static int qam_args(int32_t m, int64_t E, int64_t batch, int64_t* S, double* scale) {
    if (int rc = pl_qam_check(m, E, S, scale)) return rc;
    if (batch < 0) return fail(PL_EINVAL, "batch must be >= 0");
    return PL_OK;
}

// sigma of an Es/N0 in dB, the expression order of pl_awgn_llr
static int qam_sigma(double snr_db, double* sigma) {
    if (!std::isfinite(snr_db)) return fail(PL_EINVAL, "snr_db must be finite");
    const double snr_linear = std::pow(10.0, snr_db / 10.0);
    *sigma = std::sqrt(1.0 / (2.0 * snr_linear));
    return PL_OK;
}

extern "C" int pl_qam_modulate(int32_t m, int64_t E, int64_t batch, const uint8_t* e, int64_t ld_e, double* x,
                               int64_t ld_x, void* stream) {
    int64_t S;
    double scale;
    if (int rc = qam_args(m, E, batch, &S, &scale)) return rc;
    if (batch > 0 && (!e || !x)) return fail(PL_EINVAL, "device pointers must not be NULL");
    if ((uintptr_t)x & 7) return fail(PL_EINVAL, "x_dev must be aligned to its element type");
    if (ld_e < E) return fail(PL_EINVAL, "ld_e < E = " + std::to_string(E));
    if (ld_x < 2 * S) return fail(PL_EINVAL, "ld_x < 2 S = " + std::to_string(2 * S));
    const hipError_t err = pl::qam_modulate_launch(m, E, S, scale, e, ld_e, batch, x, ld_x, (hipStream_t)stream);
    return err == hipSuccess ? PL_OK : hipfail(err, "qam modulate launch");
}

extern "C" int pl_qam_awgn(int32_t m, int64_t E, int64_t batch, const uint8_t* e, int64_t ld_e, double snr_db,
                           uint64_t seed, int64_t frame_offset, double* y, int64_t ld_y, void* stream) {
    int64_t S;
    double scale, sigma;
    if (int rc = qam_args(m, E, batch, &S, &scale)) return rc;
    if (batch > 0 && !y) return fail(PL_EINVAL, "y_dev must not be NULL");
    if (int rc = qam_sigma(snr_db, &sigma)) return rc;
    if ((uintptr_t)y & 7) return fail(PL_EINVAL, "y_dev must be aligned to its element type");
    if (e && ld_e < E) return fail(PL_EINVAL, "ld_e < E = " + std::to_string(E));
    if (ld_y < 2 * S) return fail(PL_EINVAL, "ld_y < 2 S = " + std::to_string(2 * S));
    const hipError_t err = pl::qam_awgn_launch(m, E, S, scale, e, ld_e, batch, sigma, seed, frame_offset, y, ld_y,
                                               (hipStream_t)stream);
    return err == hipSuccess ? PL_OK : hipfail(err, "qam awgn launch");
}

// pl_qam_demap and pl_qam_demap_logmap: one argument list, one set of refusals, the kernel by `logmap`
static int qam_demap_call(bool logmap, int32_t m, int64_t E, int64_t batch, const double* y, int64_t ld_y,
                          double snr_db, void* llr, int64_t ld_llr, int32_t flags, void* stream) {
    int64_t S;
    double scale, sigma;
    if (int rc = qam_args(m, E, batch, &S, &scale)) return rc;
    if (batch > 0 && (!y || !llr)) return fail(PL_EINVAL, "device pointers must not be NULL");
    if (flags & ~PL_QAM_LLR_F32) return fail(PL_EINVAL, "unknown flag bits");
    if (int rc = qam_sigma(snr_db, &sigma)) return rc;
    if (((uintptr_t)y & 7) || ((uintptr_t)llr & ((flags & PL_QAM_LLR_F32) ? 3 : 7)))
        return fail(PL_EINVAL, "y_dev and llr_dev must be aligned to their element type");
    if (ld_y < 2 * S) return fail(PL_EINVAL, "ld_y < 2 S = " + std::to_string(2 * S));
    if (ld_llr < E) return fail(PL_EINVAL, "ld_llr < E = " + std::to_string(E));
    const double s2 = sigma * sigma;
    const double w = 1.0 / (2.0 * s2);
    const hipError_t err =
        logmap ? pl::qam_demap_logmap_launch(m, E, S, 1, scale, y, ld_y, nullptr, 0, batch, w, llr, ld_llr,
                                             flags & PL_QAM_LLR_F32, (hipStream_t)stream)
               : pl::qam_demap_launch(m, E, S, scale, y, ld_y, batch, w, llr, ld_llr, flags & PL_QAM_LLR_F32,
                                      (hipStream_t)stream);
    return err == hipSuccess ? PL_OK : hipfail(err, logmap ? "qam demap logmap launch" : "qam demap launch");
}

extern "C" int pl_qam_demap(int32_t m, int64_t E, int64_t batch, const double* y, int64_t ld_y, double snr_db,
                            void* llr, int64_t ld_llr, int32_t flags, void* stream) {
    return qam_demap_call(false, m, E, batch, y, ld_y, snr_db, llr, ld_llr, flags, stream);
}

extern "C" int pl_qam_demap_logmap(int32_t m, int64_t E, int64_t batch, const double* y, int64_t ld_y, double snr_db,
                                   void* llr, int64_t ld_llr, int32_t flags, void* stream) {
    return qam_demap_call(true, m, E, batch, y, ld_y, snr_db, llr, ld_llr, flags, stream);
}

// ---- block Rayleigh fading for the QAM symbols (qam.hip); the definition: include/polarldpc.h, pl_qam_fading_check ----
extern "C" int pl_qam_fading_check(int32_t m, int64_t E, int64_t coherence, int64_t* S, int64_t* Q) {
    const pl::QamStatus st = pl::qam_fading_check(m, E, coherence, S, Q);
    return st.code ? fail(st.code, st.msg) : PL_OK;
}

// what the two entry points share behind the parameters, every check before the first device call
static int qam_fading_buffers(int64_t batch, const double* y, int64_t ld_y, const double* h, int64_t ld_h, int64_t S,
                              int64_t Q) {
    if (batch < 0) return fail(PL_EINVAL, "batch must be >= 0");
    if (batch > 0 && !y) return fail(PL_EINVAL, "y_dev must not be NULL");
    if (batch > 0 && !h) return fail(PL_EINVAL, "h_dev must not be NULL");
    if (((uintptr_t)y | (uintptr_t)h) & 7) return fail(PL_EINVAL, "y_dev and h_dev must be aligned to their element type");
    if (ld_y < 2 * S) return fail(PL_EINVAL, "ld_y < 2 S = " + std::to_string(2 * S));
    if (ld_h < 2 * Q) return fail(PL_EINVAL, "ld_h < 2 Q = " + std::to_string(2 * Q));
    return PL_OK;
}

extern "C" int pl_qam_rayleigh(int32_t m, int64_t E, int64_t coherence, int64_t batch, const uint8_t* e, int64_t ld_e,
                               double snr_db, uint64_t seed, int64_t frame_offset, double* y, int64_t ld_y, double* h,
                               int64_t ld_h, void* stream) {
    int64_t S, Q;
    double scale, sigma;
    if (int rc = pl_qam_fading_check(m, E, coherence, &S, &Q)) return rc;
    if (int rc = qam_fading_buffers(batch, y, ld_y, h, ld_h, S, Q)) return rc;
    if (int rc = qam_sigma(snr_db, &sigma)) return rc;
    if (e && ld_e < E) return fail(PL_EINVAL, "ld_e < E = " + std::to_string(E));
    pl::qam_check(m, E, nullptr, &scale);
    const hipError_t err = pl::qam_rayleigh_launch(m, E, S, coherence, scale, e, ld_e, batch, sigma, seed, frame_offset,
                                                   y, ld_y, h, ld_h, (hipStream_t)stream);
    return err == hipSuccess ? PL_OK : hipfail(err, "qam rayleigh launch");
}

// pl_qam_demap_csi and pl_qam_demap_csi_logmap, as qam_demap_call
static int qam_demap_csi_call(bool logmap, int32_t m, int64_t E, int64_t coherence, int64_t batch, const double* y,
                              int64_t ld_y, const double* h, int64_t ld_h, double snr_db, void* llr, int64_t ld_llr,
                              int32_t flags, void* stream) {
    int64_t S, Q;
    double scale, sigma;
    if (int rc = pl_qam_fading_check(m, E, coherence, &S, &Q)) return rc;
    if (int rc = qam_fading_buffers(batch, y, ld_y, h, ld_h, S, Q)) return rc;
    if (batch > 0 && !llr) return fail(PL_EINVAL, "llr_dev must not be NULL");
    if (flags & ~PL_QAM_LLR_F32) return fail(PL_EINVAL, "unknown flag bits");
    if (int rc = qam_sigma(snr_db, &sigma)) return rc;
    if ((uintptr_t)llr & ((flags & PL_QAM_LLR_F32) ? 3 : 7))
        return fail(PL_EINVAL, "llr_dev must be aligned to its element type");
    if (ld_llr < E) return fail(PL_EINVAL, "ld_llr < E = " + std::to_string(E));
    pl::qam_check(m, E, nullptr, &scale);
    const double s2 = sigma * sigma;
    const double w = 1.0 / (2.0 * s2);
    const hipError_t err = (logmap ? pl::qam_demap_logmap_launch : pl::qam_demap_csi_launch)(
        m, E, S, coherence, scale, y, ld_y, h, ld_h, batch, w, llr, ld_llr, flags & PL_QAM_LLR_F32, (hipStream_t)stream);
    return err == hipSuccess ? PL_OK : hipfail(err, logmap ? "qam demap csi logmap launch" : "qam demap csi launch");
}

extern "C" int pl_qam_demap_csi(int32_t m, int64_t E, int64_t coherence, int64_t batch, const double* y, int64_t ld_y,
                                const double* h, int64_t ld_h, double snr_db, void* llr, int64_t ld_llr, int32_t flags,
                                void* stream) {
    return qam_demap_csi_call(false, m, E, coherence, batch, y, ld_y, h, ld_h, snr_db, llr, ld_llr, flags, stream);
}

extern "C" int pl_qam_demap_csi_logmap(int32_t m, int64_t E, int64_t coherence, int64_t batch, const double* y,
                                       int64_t ld_y, const double* h, int64_t ld_h, double snr_db, void* llr,
                                       int64_t ld_llr, int32_t flags, void* stream) {
    return qam_demap_csi_call(true, m, E, coherence, batch, y, ld_y, h, ld_h, snr_db, llr, ld_llr, flags, stream);
}

// ---- the bit interleaver (interleave.hip); the definition: include/polarldpc.h, pl_interleave_check ----
static int ilv_args(int32_t kind, int32_t rows, int64_t E, pl::IlvParams* p) {
    const pl::IlvStatus st = pl::ilv_check(kind, rows, E, p);
    return st.code ? fail(st.code, st.msg) : PL_OK;
}

extern "C" int pl_interleave_check(int32_t kind, int32_t rows, int64_t E, int64_t* dim) {
    pl::IlvParams p;
    if (int rc = ilv_args(kind, rows, E, &p)) return rc;
    if (dim) *dim = p.dim;
    return PL_OK;
}

extern "C" int pl_interleave_index(int32_t kind, int32_t rows, int64_t E, int64_t k, int64_t* pos) {
    pl::IlvParams p;
    if (int rc = ilv_args(kind, rows, E, &p)) return rc;
    if (k < 0 || k >= E) return fail(PL_EINVAL, "k = " + std::to_string(k) + " outside 0 .. E-1");
    if (!pos) return fail(PL_EINVAL, "pos_out must not be NULL");
    *pos = pl::ilv_pos(kind, p, (uint32_t)k);
    return PL_OK;
}

extern "C" int64_t pl_interleave_lds_max_e(int32_t elem_size) {
    return elem_size == 1 || elem_size == 4 || elem_size == 8 ? pl::kIlvLdsBytes / elem_size : 0;
}

// what the two entry points share, every check before the first device call; size: bytes per element
static int ilv_buffers(int64_t E, int64_t batch, const void* e, int64_t ld_e, const void* f, int64_t ld_f, int size) {
    if (batch < 0) return fail(PL_EINVAL, "batch must be >= 0");
    if (batch > 0 && (!e || !f)) return fail(PL_EINVAL, "device pointers must not be NULL");
    if (((uintptr_t)e | (uintptr_t)f) & (uintptr_t)(size - 1))
        return fail(PL_EINVAL, "e_dev and f_dev must be aligned to their element type");
    if (ld_e < E) return fail(PL_EINVAL, "ld_e < E = " + std::to_string(E));
    if (ld_f < E) return fail(PL_EINVAL, "ld_f < E = " + std::to_string(E));
    if (batch > 0) {
        // the bytes each side spans, rows and the gaps between them: [e, e + ne) against [f, f + nf)
        const unsigned __int128 ne = ((unsigned __int128)(batch - 1) * ld_e + E) * size;
        const unsigned __int128 nf = ((unsigned __int128)(batch - 1) * ld_f + E) * size;
        const unsigned __int128 e0 = (uintptr_t)e, f0 = (uintptr_t)f;
        if (e0 < f0 + nf && f0 < e0 + ne) return fail(PL_EINVAL, "e_dev and f_dev overlap");
    }
    return PL_OK;
}

extern "C" int pl_bit_interleave(int32_t kind, int32_t rows, int64_t E, int64_t batch, const uint8_t* e, int64_t ld_e,
                                 uint8_t* f, int64_t ld_f, void* stream) {
    pl::IlvParams p;
    if (int rc = ilv_args(kind, rows, E, &p)) return rc;
    if (int rc = ilv_buffers(E, batch, e, ld_e, f, ld_f, 1)) return rc;
    const hipError_t err = pl::bit_interleave_launch(kind, p, e, ld_e, batch, f, ld_f, (hipStream_t)stream);
    return err == hipSuccess ? PL_OK : hipfail(err, "bit interleave launch");
}

extern "C" int pl_llr_deinterleave(int32_t kind, int32_t rows, int64_t E, int64_t batch, const void* f, int64_t ld_f,
                                   void* e, int64_t ld_e, int32_t flags, void* stream) {
    pl::IlvParams p;
    if (int rc = ilv_args(kind, rows, E, &p)) return rc;
    if (flags & ~PL_ILV_LLR_F32) return fail(PL_EINVAL, "unknown flag bits");
    const bool f32 = flags & PL_ILV_LLR_F32;
    if (int rc = ilv_buffers(E, batch, e, ld_e, f, ld_f, f32 ? 4 : 8)) return rc;
    const hipError_t err = pl::llr_deinterleave_launch(kind, p, f, ld_f, batch, e, ld_e, f32, (hipStream_t)stream);
    return err == hipSuccess ? PL_OK : hipfail(err, "llr deinterleave launch");
}

extern "C" int pl_count_errors(const uint8_t* ref, int64_t ldr, const uint8_t* dec, int64_t ldd, int32_t width,
                               int64_t batch, int64_t* counts, void* stream) {
    if (batch < 0 || width < 0 || !counts || (batch > 0 && (!ref || !dec))) return fail(PL_EINVAL, "bad argument");
    hipError_t e = pl::count_errors_launch(ref, ldr, dec, ldd, width, batch, counts, (hipStream_t)stream);
    return e == hipSuccess ? PL_OK : hipfail(e, "count errors launch");
}

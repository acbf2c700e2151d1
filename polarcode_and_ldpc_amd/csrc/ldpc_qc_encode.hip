// Encoder for quasi-cyclic LDPC codes from the base matrix on gfx950 (MI355X):
// valid codewords of the code ldpc_qc_layered.hip decodes, by cyclic shifts and
// XORs in block-row order.  No generator, H is never expanded.  The supported
// structure of the parity part (a core of g block rows, then a lower-triangular
// extension) and the encoding steps 1-5: include/polarldpc.h,
// pl_ldpc_qc_encoder_create; the stream this kernel walks: ldpc_plan.hpp,
// QcEncHostPlan.
// Mapping, as the decoder's: one thread per check of the current block row; the
// bit check r reads through the block (col, s) is col Z + (r + s >= Z ? r + s -
// Z : r + s): consecutive lanes, consecutive bytes.
//   SUBWAVE (Z <= 64): fpw = 64 / Z frames share a wavefront, lane l = frame
//     l / Z, check l % Z; up to four wavefronts per workgroup, each on its own
//     LDS slice, ordered by the wavefront-level fence only: no workgroup barrier.
//     Lanes past fpw Z and frames past the batch compute on the wavefront's
//     first frame and store nothing.
//   block (Z > 64): one frame per workgroup of roundup64(Z) threads; behind the
//     message load and p_0, then __syncthreads only where the stream's sync flag
//     says so, and one before the codeword goes out.
// Per frame the LDS holds the codeword C[n], one byte per bit (C[0:k] is the
// message, bytes taken & 1 on load), and behind it lambda_t[Z] for the g core
// rows.  The stream is the only table, read at wave-uniform addresses; global
// memory is read for the message and written for the codeword, nothing else.
// Rows move in 16-byte pieces when the pointer and the pitch allow (VIN / VOUT),
// else byte by byte; both in whole wavefronts, so idle lanes help with the copy.
#include "common.hpp"
#include "internal.hpp"
#include "ldpc_lms_check.hpp"

namespace pl {

// The stream, in the constant address space: never written while a kernel runs, and read at wave-uniform
// addresses only, so every load of it is a scalar load whatever LDS stores and fences lie in between.
typedef const int32_t __attribute__((address_space(4))) qce_word;
PL_DEV qce_word* qce_stream(const int32_t* tab) {
    return (qce_word*)tab;  // generic -> constant: the same address
}

// position in its block column of the bit check r reads through a block of shift s
PL_DEV int qce_rot(int r, int s, int z) {
    const int t = r + s;
    return t >= z ? t - z : t;
}

// XOR over d (block column, shift) pairs of the bits check r reads
PL_DEV uint32_t qce_row_sum(const unsigned char* C, qce_word* pr, int d, int r, int z) {
    uint32_t acc = 0;
    for (int j = 0; j < d; ++j) acc ^= C[pr[2 * j] * z + qce_rot(r, pr[2 * j + 1], z)];
    return acc;
}

// message row -> LDS, bytes & 1; `tid` of `nthr` threads; dst 16-byte aligned.  The loops of qce_load and
// qce_store stride by nthr >= 64: not vectorised, or the compiler adds a dead nthr == 1 version of each
template <bool VEC>
PL_DEV void qce_load(unsigned char* dst, const uint8_t* __restrict__ src, int k, int tid, int nthr) {
    int done = 0;
    if (VEC) {
        const int k16 = k >> 4;
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
        uint4* d4 = reinterpret_cast<uint4*>(dst);
#pragma clang loop vectorize(disable) interleave(disable)
        for (int i = tid; i < k16; i += nthr) {
            uint4 v = s4[i];
            v.x &= 0x01010101u; v.y &= 0x01010101u; v.z &= 0x01010101u; v.w &= 0x01010101u;
            d4[i] = v;
        }
        done = k16 << 4;
    }
#pragma clang loop vectorize(disable) interleave(disable)
    for (int i = done + tid; i < k; i += nthr) dst[i] = src[i] & 1;
}

// LDS -> codeword row; src 16-byte aligned
template <bool VEC>
PL_DEV void qce_store(uint8_t* __restrict__ dst, const unsigned char* src, int n, int tid, int nthr) {
    int done = 0;
    if (VEC) {
        const int n16 = n >> 4;
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
        uint4* d4 = reinterpret_cast<uint4*>(dst);
#pragma clang loop vectorize(disable) interleave(disable)
        for (int i = tid; i < n16; i += nthr) d4[i] = s4[i];
        done = n16 << 4;
    }
#pragma clang loop vectorize(disable) interleave(disable)
    for (int i = done + tid; i < n; i += nthr) dst[i] = src[i];
}

template <bool SUBWAVE, bool VIN, bool VOUT>
__global__ void __launch_bounds__(SUBWAVE ? 256 : 1024)
ldpc_qc_encode_kernel(QcEncGeom g, const int32_t* __restrict__ tab, const uint8_t* __restrict__ msg, int64_t ldm,
                      int64_t batch, uint8_t* __restrict__ cw, int64_t ldc) {
    extern __shared__ __align__(16) unsigned char qce_smem[];
    const int z = g.z;
    int r;
    bool mine;          // this lane holds check r of a frame of the batch
    unsigned char* C;   // the lane's frame
    unsigned char* W;   // SUBWAVE: the wavefront's first frame
    int64_t frame0;     // the first frame of the wavefront / the workgroup's frame
    int nf = 1;         // frames of the wavefront within the batch
    const int lane = (int)(threadIdx.x & 63u);
    if (SUBWAVE) {
        const int wv = (int)(threadIdx.x >> 6);
        frame0 = ((int64_t)blockIdx.x * g.fpb + wv) * g.fpw;
        if (frame0 >= batch) return;  // a ragged last workgroup (no workgroup barrier below)
        nf = (int)(batch - frame0 < (int64_t)g.fpw ? batch - frame0 : (int64_t)g.fpw);
        const int f = lane / z;
        mine = f < nf;
        r = mine ? lane - f * z : 0;
        W = qce_smem + (size_t)wv * (size_t)g.fpw * (size_t)g.frame_bytes;
        C = W + (size_t)(mine ? f : 0) * (size_t)g.frame_bytes;
        for (int ff = 0; ff < nf; ++ff)
            qce_load<VIN>(W + (size_t)ff * (size_t)g.frame_bytes, msg + (frame0 + ff) * ldm, g.k, lane, 64);
    } else {
        frame0 = (int64_t)blockIdx.x;
        mine = (int)threadIdx.x < z;
        r = mine ? (int)threadIdx.x : 0;
        W = C = qce_smem;
        qce_load<VIN>(C, msg + frame0 * ldm, g.k, (int)threadIdx.x, (int)blockDim.x);
    }
    unsigned char* const LAM = C + g.n;
    lms_sync<SUBWAVE>();

    qce_word* t = qce_stream(tab);
    const int G = t[0], x = t[1], a = t[2], b = t[3];
    t += 4;
    if (G > 0) {
        unsigned char* const p0 = C + g.kb * z;
        uint32_t sum = 0;  // p_0[(r + b) % Z]
        for (int i = 0; i < G; ++i) {
            const int d = t[0];
            const uint32_t lam = qce_row_sum(C, t + 1, d, r, z);
            t += 1 + 2 * d;
            if (mine) LAM[i * z + r] = (unsigned char)lam;
            sum ^= lam;
        }
        if (mine) p0[qce_rot(r, b, z)] = (unsigned char)sum;
        lms_sync<SUBWAVE>();
        // the chain stays in lane r: lambda_t[r] and p_t[r] are this lane's own stores
        uint32_t p = LAM[r] ^ p0[qce_rot(r, a, z)];
        if (mine) p0[z + r] = (unsigned char)p;
        for (int i = 1; i <= G - 2; ++i) {
            p ^= LAM[i * z + r] ^ (i == x ? sum : 0u);
            if (mine) p0[(i + 1) * z + r] = (unsigned char)p;
        }
    }
    for (int i = G; i < g.mb; ++i) {
        const int di = t[0], sync = t[1], d = t[2];
        if (sync) lms_sync<SUBWAVE>();  // the same in every lane
        const uint32_t acc = qce_row_sum(C, t + 3, d, r, z);
        t += 3 + 2 * d;
        if (mine) C[(g.kb + i) * z + qce_rot(r, di, z)] = (unsigned char)acc;
    }
    lms_sync<SUBWAVE>();

    if (SUBWAVE) {
        for (int ff = 0; ff < nf; ++ff)
            qce_store<VOUT>(cw + (frame0 + ff) * ldc, W + (size_t)ff * (size_t)g.frame_bytes, g.n, lane, 64);
    } else {
        qce_store<VOUT>(cw + frame0 * ldc, C, g.n, (int)threadIdx.x, (int)blockDim.x);
    }
}

template <bool SUBWAVE>
static void* qce_pick_io(bool vin, bool vout) {
    if (vin) return vout ? (void*)ldpc_qc_encode_kernel<SUBWAVE, true, true> : (void*)ldpc_qc_encode_kernel<SUBWAVE, true, false>;
    return vout ? (void*)ldpc_qc_encode_kernel<SUBWAVE, false, true> : (void*)ldpc_qc_encode_kernel<SUBWAVE, false, false>;
}
static void* qce_pick(const QcEncGeom& g, bool vin, bool vout) {
    return g.subwave ? qce_pick_io<true>(vin, vout) : qce_pick_io<false>(vin, vout);
}

hipError_t qc_encode_prepare(const QcEncGeom& g) {
    for (int v = 0; v < 4; ++v) {
        const hipError_t e = hipFuncSetAttribute(qce_pick(g, v & 1, v & 2), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 g.lds_bytes);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t qc_encode_launch(const QcEncGeom& g, const int32_t* tab, const uint8_t* msg, int64_t ldm, int64_t batch,
                            uint8_t* cw, int64_t ldc, hipStream_t s) {
    if (batch == 0) return hipSuccess;
    // 16-byte pieces: every row starts on a 16-byte boundary (batch 1: the pitch is not used)
    const bool vin = ((uintptr_t)msg & 15) == 0 && (batch == 1 || ldm % 16 == 0);
    const bool vout = ((uintptr_t)cw & 15) == 0 && (batch == 1 || ldc % 16 == 0);
    QcEncGeom gg = g;
    const int64_t fpg = (int64_t)g.fpw * g.fpb;  // frames per workgroup
    void* args[] = {&gg, (void*)&tab, (void*)&msg, (void*)&ldm, (void*)&batch, (void*)&cw, (void*)&ldc};
    return hipLaunchKernel(qce_pick(g, vin, vout), dim3((unsigned)((batch + fpg - 1) / fpg)), dim3(g.threads), args,
                           g.lds_bytes, s);
}

}  // namespace pl

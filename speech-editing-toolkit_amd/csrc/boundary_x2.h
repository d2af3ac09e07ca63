// The step-boundary kernels of the reverse loop (csrc/boundary.hip): the two-piece fp16 GEMM of the step boundary (skip projection, output
// head, next step's input projection; diffnet.py:118-120,128-131, spec_denoiser.py:86-101).  The posterior's noise comes from philox.h.
#pragma once
#include "common.h"
#include "philox.h"

namespace {

constexpr int BX_DC = 256;             // residual channels
constexpr int BX_XR = BX_DC * 2 + 16;     // bytes per row of the s / h tiles [frame][256]
constexpr int BX_PR = 96 * 2 + 16;     // ... of the x' tile [frame][96]
constexpr int BX_PIECE = 64 * BX_XR;   // one piece of a [64][256] tile

__device__ __forceinline__ void bx_split(float v, unsigned short &p0, unsigned short &p1) {
    const _Float16 h0 = (_Float16)v;
    p0 = __builtin_bit_cast(unsigned short, h0);
    p1 = __builtin_bit_cast(unsigned short, (_Float16)(v - (float)h0));
}
// acc[NRB][2] += W[32 (rb0 + i) .. ][16 ks ..] * B over nks k-steps; image [rb32][ng16][piece][lane][8] (K = 1 tap);
// B piece q of (ks, cb) at lds + q * piece_bytes + bfrag(ks, cb)
template <int NRB, typename BF>
__device__ __forceinline__ void bx_gemm(f32x16 (&acc)[NRB][2], rsrc_t img, unsigned lane16, int rb0, int ng16, int nks,
                                        const unsigned char *lds, unsigned piece_bytes, BF bfrag) {
    // Weight fragments straight from the packed image through a ring of PF k-steps, the k-step order pinned (round 4, as in gemm_x3 /
    // sx_gemm):  ds_read B(k + 1) | the MFMAs of k-step k straight from their ring slot | refill of that slot | sched_barrier.  Rounds 2-3
    // had `Ac = A[p]; A[p] = load; mma(Ac)` with a ring of 2: 150 of the kernel's 312 MFMAs sat right behind an s_waitcnt vmcnt(0 / 1).
    // Same products in the same order per accumulator: bit-identical.
    constexpr int PF = 4;
    auto a_load = [&](int ks, int i, int q) {
        return (u32x4_t)__builtin_amdgcn_raw_buffer_load_b128(img, (int)lane16, (int)((((rb0 + i) * ng16 + ks) * 2 + q) * 1024), 0);
    };
    u32x4_t A[PF][NRB][2];
#pragma unroll
    for (int p = 0; p < PF; ++p)
#pragma unroll
        for (int i = 0; i < NRB; ++i)
#pragma unroll
            for (int q = 0; q < 2; ++q) A[p][i][q] = a_load(min(p, nks - 1), i, q);
    u32x4_t Bv[2][2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const unsigned bo = bfrag(0, cb);
        Bv[cb][0] = *reinterpret_cast<const u32x4_t *>(lds + bo);
        Bv[cb][1] = *reinterpret_cast<const u32x4_t *>(lds + piece_bytes + bo);
    }
#pragma unroll 1
    for (int kb = 0; kb < nks; kb += PF) {
#pragma unroll
        for (int p = 0; p < PF; ++p) {
            const int ks = kb + p;
            if (ks < nks) {  // (nks need not be a multiple of PF: the in-projection has 5 k-steps)
                u32x4_t Bn[2][2];
                const int kq = min(ks + 1, nks - 1);
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    const unsigned bo = bfrag(kq, cb);
                    Bn[cb][0] = *reinterpret_cast<const u32x4_t *>(lds + bo);
                    Bn[cb][1] = *reinterpret_cast<const u32x4_t *>(lds + piece_bytes + bo);
                }
#pragma unroll
                for (int t = 0; t < 3; ++t)  // a1 b0, a0 b1, a0 b0
#pragma unroll
                    for (int i = 0; i < NRB; ++i)
#pragma unroll
                        for (int cb = 0; cb < 2; ++cb) acc[i][cb] = mfma_f16(A[p][i][t == 0 ? 1 : 0], Bv[cb][t == 1 ? 1 : 0], acc[i][cb]);
                const int kn = min(ks + PF, nks - 1);
#pragma unroll
                for (int i = 0; i < NRB; ++i) {
                    A[p][i][0] = a_load(kn, i, 0);
                    A[p][i][1] = a_load(kn, i, 1);
                }
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) {
                    Bv[cb][0] = Bn[cb][0];
                    Bv[cb][1] = Bn[cb][1];
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}


}  // namespace

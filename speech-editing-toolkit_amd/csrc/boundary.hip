// The step boundary of the reverse diffusion loop for gfx950: diffnet_boundary_kernel (fp32 MFMA pipe), diffnet_boundary_x2_kernel (two-piece
// fp16 operands) and their launch (launch_boundary, called by csrc/diffusion_loop.hip).
//
// Step boundary: everything between the layer stack of step k and the layer stack of step k+1 in ONE launch:
//   h   = ReLU(W_skip * (skip / sqrt(L)) + b_skip)            (diffnet.py:128-130)
//   x0  = W_out * h + b_out                                    (diffnet.py:131)
//   x'  = c1 x0 + c2 x_t + nonzero * exp(logvar/2) * eps       (spec_denoiser.py:86-101, eps explicit or Philox)
//   xin = ReLU(W_in * x' + b_in)                               (diffnet.py:118-120, input of the next step)
// One block = one utterance x 64 frames, 4 waves, everything stays in LDS/registers between the three GEMMs.  The
// four separate launches this replaces were latency-bound (31 + 75 + 51 + 14 us at B=32, T=800).  Weights are the
// ordinary packed conv images (set_pack_conv_weight); arithmetic order (prologue divide, bias after the sum, Philox
// quad = 4 consecutive frames of one row, the device word of set_rng_seed_delta added to the seed) equals the unfused kernels, so
// results are bit-identical to them.
// Needs T % 4 == 0 (quad alignment), 256 residual channels, M <= 96 mel bins.
// ----------------------------------------------------------------------------------------------------------
#include <stdlib.h>

#include "common.h"
#include "boundary_x2.h"
#include "diffnet_host.h"

namespace {
constexpr int DC = 256;  // residual_channels these kernels are specialised for
}

struct BoundaryArgs {
    const float *skip;      // [B][256][T]
    float *x;               // [B][M][T]  in: x_t, out: x_{t-1}
    const float *eps;       // [B][M][T] or NULL
    const float *coef4;     // {c1, c2, logvar, nonzero} of this step (device)
    const float *w_skip_p, *b_skip, *w_outp_p, *b_outp, *w_in_p, *b_in;
    float *xin_next;        // [B][256][T] or NULL (last step)
    float inv_div;          // unused (division by sqrt(L) is done exactly as the conv prologue does: x / p)
    float div;
    uint64_t seed, quad_offset;
    const uint64_t *seed_delta;  // set_rng_seed_delta (may be NULL): added to the seed, as set_posterior_step does
    int T, M, MP;           // MP = M rounded up to 16 (rows of the x' tile in LDS, K of the head GEMM)
};
constexpr int BD_LD = 64;

__global__ void __launch_bounds__(256, 2) diffnet_boundary_kernel(BoundaryArgs a) {
    extern __shared__ __attribute__((aligned(16))) float smem[];  // [256][64]: skip tile -> h tile -> x' tile
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.y, t0 = blockIdx.x * 64, T = a.T, M = a.M;
    // ---- phase 1: skip tile / sqrt(L) -> LDS (wave w: rows 64w .. 64w+63, lanes along t; unconditional clamped loads)
    {
        const rsrc_t rs = make_rsrc(a.skip + (int64_t)b * DC * T);
        const unsigned vo = 4u * (unsigned)min(t0 + lane, T - 1);
        const bool tv = t0 + lane < T;
        for (int r0 = 0; r0 < 64; r0 += 16) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) v[u] = buf_load(rs, vo, 4u * (unsigned)(64 * w + r0 + u) * (unsigned)T);
#pragma unroll
            for (int u = 0; u < 16; ++u) smem[(64 * w + r0 + u) * BD_LD + lane] = tv ? v[u] / a.div : 0.0f;
        }
    }
    __syncthreads();
    // ---- phase 2: h = ReLU(W_skip * s + b): wave w owns rows [64w, 64w+64) = row blocks 2w, 2w+1
    f32x16 acc[2][1][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        acc[i][0][0] = (f32x16){0};
        acc[i][0][1] = (f32x16){0};
        const float *wp = a.w_skip_p + (int64_t)(2 * w + i) * (DC / 2) * 64 + lane;
        const float *bp = smem + half * BD_LD + l31;
        gemm_groups<1, 2, 8>(acc[i], wp, bp, 2 * BD_LD, (DC / 2) / 8, [&](int) {
            wp += 8 * 64;
            bp += 8 * 2 * BD_LD;
        });
    }
    __syncthreads();  // every wave is done reading the skip tile
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = 32 * (2 * w + i) + mfma32_row(r, lane);
            const float bias = a.b_skip[row];
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) smem[row * BD_LD + 32 * cb + l31] = fmaxf(acc[i][0][cb][r] + bias, 0.0f);
        }
    __syncthreads();
    // ---- phase 3: x0 = W_out * h + b: row blocks 0..ceil(M/32)-1 on waves 0..2
    const int rbn = (M + 31) / 32;
    f32x16 xo[1][2];
    xo[0][0] = (f32x16){0};
    xo[0][1] = (f32x16){0};
    if (w < rbn) {
        const float *wp = a.w_outp_p + (int64_t)w * (DC / 2) * 64 + lane;
        const float *bp = smem + half * BD_LD + l31;
        gemm_groups<1, 2, 8>(xo, wp, bp, 2 * BD_LD, (DC / 2) / 8, [&](int) {
            wp += 8 * 64;
            bp += 8 * 2 * BD_LD;
        });
    }
    __syncthreads();  // h tile consumed
    if (w < rbn) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = 32 * w + mfma32_row(r, lane);
            const float bias = a.b_outp[min(row, M - 1)];
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) smem[row * BD_LD + 32 * cb + l31] = row < M ? xo[0][cb][r] + bias : 0.0f;
        }
    }
    __syncthreads();
    // ---- phase 4: posterior update on quads of 4 consecutive frames (T % 4 == 0: a quad never straddles rows)
    {
        const float c1 = a.coef4[0], c2 = a.coef4[1], sig = a.coef4[3] * expf(0.5f * a.coef4[2]);
        uint64_t seed = a.seed;
        if (a.seed_delta) seed += *a.seed_delta;  // set_rng_seed_delta: see randn_kernel (one wave-uniform load)
        float *xb = a.x + (int64_t)b * M * T;
        const float *eb = a.eps ? a.eps + (int64_t)b * M * T : nullptr;
        for (int qi = tid; qi < a.MP * 16; qi += 256) {
            const int m = qi >> 4, tq = qi & 15, t = t0 + 4 * tq;
            float *cell = smem + m * BD_LD + 4 * tq;
            if (m < M && t < T) {
                const int64_t i = (int64_t)m * T + t;
                const f32x4 xt = *reinterpret_cast<const f32x4 *>(xb + i);
                float z[4];
                if (eb) {
                    const f32x4 e4 = *reinterpret_cast<const f32x4 *>(eb + i);
                    z[0] = e4[0]; z[1] = e4[1]; z[2] = e4[2]; z[3] = e4[3];
                } else {
                    randn4(seed, a.quad_offset + (uint64_t)(((int64_t)b * M * T + i) >> 2), z);
                }
                f32x4 o;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float mean = c1 * cell[k] + c2 * xt[k];
                    o[k] = mean + sig * z[k];
                }
                *reinterpret_cast<f32x4 *>(xb + i) = o;
                *reinterpret_cast<f32x4 *>(cell) = o;
            } else {
                *reinterpret_cast<f32x4 *>(cell) = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};  // K padding rows / frames >= T
            }
        }
    }
    if (!a.xin_next) return;
    __syncthreads();
    // ---- phase 5: next step's input projection xin = ReLU(W_in * x' + b_in), K = MP
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        acc[i][0][0] = (f32x16){0};
        acc[i][0][1] = (f32x16){0};
        const float *wp = a.w_in_p + (int64_t)(2 * w + i) * (a.MP / 2) * 64 + lane;
        const float *bp = smem + half * BD_LD + l31;
        gemm_groups<1, 2, 4>(acc[i], wp, bp, 2 * BD_LD, (a.MP / 2) / 4, [&](int) {
            wp += 4 * 64;
            bp += 4 * 2 * BD_LD;
        });
    }
    const rsrc_t ro = make_rsrc(a.xin_next + (int64_t)b * DC * T);
    // all 32 bias values first: a bias load placed between the stores cannot be moved across them (b_in may alias
    // xin_next as far as the compiler knows), which serialises one L2 round trip per store
    float bin[2][16];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) bin[i][r] = (a.b_in + 32 * (2 * w + i) + urow16(r))[4 * half];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        if (t0 + 32 * cb + l31 < T) {
            const unsigned so = 4u * (unsigned)(4 * half * T + t0 + 32 * cb + l31);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int ur = 32 * (2 * w + i) + urow16(r);  // wave-uniform; + 4*half rows in the lane offset
                    buf_store(fmaxf(acc[i][0][cb][r] + bin[i][r], 0.0f), ro, so, 4u * (unsigned)ur * (unsigned)T);
                }
        }
    }
}

// ---- the same step boundary on the two-piece fp16 operands (csrc/diffnet_x3.hip, csrc/conv_x2.hip: fp32 operands as two
// fp16 pieces, three fp16 MFMAs per product, fp32 accumulate).  The fp32 kernel above is bound by its three small GEMMs on
// the fp32 MFMA pipe (23 us of pipe time per 64-frame tile); here they take a fifth of that.  Same tile, same five phases;
// the operand tiles live in LDS as [piece][frame][channel] fp16 (rows padded by 16 B), the weights come from the images of
// set_pack_conv_weight_x2 (A-fragment order, straight from global memory), x0 / x' pass through an fp32 tile for the
// posterior update exactly as above.  Used by the reverse loop whenever the layer stack runs on two-piece fp16 operands.
// (bx_split / bx_gemm and the tile constants: csrc/boundary_x2.h)
struct BoundaryX2Args {
    BoundaryArgs g;
    const unsigned short *w_skip_x2, *w_outp_x2, *w_in_x2;
    int32_t *err_flag;
};

// Q4: skip and xin_next in the channel-quad layout (common.h, q4f_index) -- phase 1 reads 16 quads of 16 bytes per lane instead of 64 floats,
// phase 5 stores its four consecutive accumulator registers as one quad.  Same values, same arithmetic.
template <bool Q4>
__global__ void __launch_bounds__(256, 2) diffnet_boundary_x2_kernel(BoundaryX2Args ax) {
    const BoundaryArgs &a = ax.g;
    extern __shared__ __attribute__((aligned(16))) unsigned char bl[];  // [2][64][BX_XR]: s -> h pieces; x0 / x' (fp32) and x' pieces overlay
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l31 = lane & 31;
    const int b = blockIdx.y, t0 = blockIdx.x * 64, T = a.T, M = a.M;
    const unsigned lane16 = 16u * (unsigned)lane;
    const unsigned T4 = 4u * (unsigned)T;
    float amax = 0.0f;
    // ---- phase 1: skip tile / sqrt(L), split -> LDS [piece][frame][256]: thread (frame f, 64 channels cg)
    {
        const int f = lane, cg = w;
        const rsrc_t rs = make_rsrc(a.skip + (int64_t)b * DC * T);
        const unsigned vo = (Q4 ? 16u : 4u) * (unsigned)min(t0 + f, T - 1);
        const bool tv = t0 + f < T;
        for (int c0 = 0; c0 < 64; c0 += 16) {
            float v[16];
            if (Q4) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 q = buf_load4(rs, vo, (unsigned)(64 * cg + c0 + 4 * j) * T4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[4 * j + e] = q[e];
                }
            } else {
#pragma unroll
                for (int u = 0; u < 16; ++u) v[u] = buf_load(rs, vo, (unsigned)(64 * cg + c0 + u) * T4);
            }
#pragma unroll
            for (int q8 = 0; q8 < 2; ++q8) {
                u32x4_t u0, u1;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    unsigned short p0[2], p1[2];
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const float sv = v[8 * q8 + 2 * e + k] / a.div;
                        const float x = tv ? sv : 0.0f;
                        amax = fmaxf(amax, fabsf(x));
                        bx_split(x, p0[k], p1[k]);
                    }
                    u0[e] = (unsigned)p0[0] | ((unsigned)p0[1] << 16);
                    u1[e] = (unsigned)p1[0] | ((unsigned)p1[1] << 16);
                }
                *reinterpret_cast<u32x4_t *>(bl + f * BX_XR + (64 * cg + c0 + 8 * q8) * 2) = u0;
                *reinterpret_cast<u32x4_t *>(bl + BX_PIECE + f * BX_XR + (64 * cg + c0 + 8 * q8) * 2) = u1;
            }
        }
    }
    __syncthreads();
    auto bfrag256 = [&](int ks, int cb) { return (unsigned)((cb * 32 + l31) * BX_XR + (ks * 16 + half * 8) * 2); };
    // ---- phase 2: h = ReLU(W_skip s + b): wave w owns rows [64w, 64w+64)
    {
        const rsrc_t rw = make_rsrc(ax.w_skip_x2);
        const float inv = reinterpret_cast<const float *>(ax.w_skip_x2 + (DC / 32) * (DC / 16) * 1024)[1];
        f32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) acc[i][cb] = (f32x16){0};
        bx_gemm<2>(acc, rw, lane16, 2 * w, DC / 16, DC / 16, bl, BX_PIECE, bfrag256);
        __syncthreads();  // every wave is done reading the s tile
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    unsigned short p0[4], p1[4];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int row = 32 * (2 * w + i) + 8 * g + 4 * half + e;
                        const float h = fmaxf(acc[i][cb][4 * g + e] * inv + a.b_skip[row], 0.0f);
                        amax = fmaxf(amax, h);
                        bx_split(h, p0[e], p1[e]);
                    }
                    const unsigned off = (unsigned)((cb * 32 + l31) * BX_XR + (32 * (2 * w + i) + 8 * g + 4 * half) * 2);
                    u32x2_t u;
                    u[0] = (unsigned)p0[0] | ((unsigned)p0[1] << 16); u[1] = (unsigned)p0[2] | ((unsigned)p0[3] << 16);
                    *reinterpret_cast<u32x2_t *>(bl + off) = u;
                    u[0] = (unsigned)p1[0] | ((unsigned)p1[1] << 16); u[1] = (unsigned)p1[2] | ((unsigned)p1[3] << 16);
                    *reinterpret_cast<u32x2_t *>(bl + BX_PIECE + off) = u;
                }
    }
    __syncthreads();
    // ---- phase 3: x0 = W_out h + b: row blocks 0 .. ceil(M/32)-1 on waves 0..2; x0 -> fp32 tile xs[96][64] (over piece 0)
    float *xs = reinterpret_cast<float *>(bl);
    {
        const int rbn = (M + 31) / 32;
        f32x16 xo[1][2];
        xo[0][0] = (f32x16){0};
        xo[0][1] = (f32x16){0};
        const float inv = reinterpret_cast<const float *>(ax.w_outp_x2 + ((M + 31) / 32) * (DC / 16) * 1024)[1];
        if (w < rbn) bx_gemm<1>(xo, make_rsrc(ax.w_outp_x2), lane16, w, DC / 16, DC / 16, bl, BX_PIECE, bfrag256);
        __syncthreads();  // h tile consumed
        if (w < 3) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 32 * w + mfma32_row(r, lane);
                const float bias = a.b_outp[min(row, M - 1)];
#pragma unroll
                for (int cb = 0; cb < 2; ++cb) xs[row * 64 + 32 * cb + l31] = (w < rbn && row < M) ? xo[0][cb][r] * inv + bias : 0.0f;
            }
        }
    }
    __syncthreads();
    // ---- phase 4: posterior update on quads of 4 consecutive frames (T % 4 == 0), as in the fp32 kernel
    {
        const float c1 = a.coef4[0], c2 = a.coef4[1], sig = a.coef4[3] * expf(0.5f * a.coef4[2]);
        uint64_t seed = a.seed;
        if (a.seed_delta) seed += *a.seed_delta;  // set_rng_seed_delta: see randn_kernel (one wave-uniform load)
        float *xb = a.x + (int64_t)b * M * T;
        const float *eb = a.eps ? a.eps + (int64_t)b * M * T : nullptr;
        for (int qi = tid; qi < 96 * 16; qi += 256) {
            const int m = qi >> 4, tq = qi & 15, t = t0 + 4 * tq;
            float *cell = xs + m * 64 + 4 * tq;
            if (m < M && t < T) {
                const int64_t i = (int64_t)m * T + t;
                const f32x4 xt = *reinterpret_cast<const f32x4 *>(xb + i);
                float z[4];
                if (eb) {
                    const f32x4 e4 = *reinterpret_cast<const f32x4 *>(eb + i);
                    z[0] = e4[0]; z[1] = e4[1]; z[2] = e4[2]; z[3] = e4[3];
                } else {
                    randn4(seed, a.quad_offset + (uint64_t)(((int64_t)b * M * T + i) >> 2), z);
                }
                f32x4 o;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float mean = c1 * cell[k] + c2 * xt[k];
                    o[k] = mean + sig * z[k];
                }
                *reinterpret_cast<f32x4 *>(xb + i) = o;
                *reinterpret_cast<f32x4 *>(cell) = o;
            } else {
                *reinterpret_cast<f32x4 *>(cell) = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};  // K padding rows / frames >= T
            }
        }
    }
    if (!a.xin_next) {
        if (!(amax < 32768.0f) && ax.err_flag) __hip_atomic_store(ax.err_flag, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    __syncthreads();
    // ---- x' (fp32 [96][64]) -> two fp16 pieces [frame][96] in the piece-1 region: thread (frame f, 24 channels cg)
    unsigned char *xp = bl + BX_PIECE;
    constexpr unsigned XP_PIECE = 64 * BX_PR;
    {
        const int f = lane, cg = w;
#pragma unroll
        for (int q8 = 0; q8 < 3; ++q8) {
            u32x4_t u0, u1;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                unsigned short p0[2], p1[2];
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const float x = xs[(24 * cg + 8 * q8 + 2 * e + k) * 64 + f];
                    amax = fmaxf(amax, fabsf(x));
                    bx_split(x, p0[k], p1[k]);
                }
                u0[e] = (unsigned)p0[0] | ((unsigned)p0[1] << 16);
                u1[e] = (unsigned)p1[0] | ((unsigned)p1[1] << 16);
            }
            *reinterpret_cast<u32x4_t *>(xp + f * BX_PR + (24 * cg + 8 * q8) * 2) = u0;
            *reinterpret_cast<u32x4_t *>(xp + XP_PIECE + f * BX_PR + (24 * cg + 8 * q8) * 2) = u1;
        }
    }
    if (!(amax < 32768.0f) && ax.err_flag) __hip_atomic_store(ax.err_flag, 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    // ---- phase 5: next step's input projection xin = ReLU(W_in x' + b_in), K = M rounded up to 32 (zero padded)
    {
        const int ngin = ((M + 31) / 32) * 2;  // 16-channel groups of the image (Cin = M rounded up to 32, zero padded)
        const float inv = reinterpret_cast<const float *>(ax.w_in_x2 + (DC / 32) * ngin * 1024)[1];
        f32x16 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb) acc[i][cb] = (f32x16){0};
        bx_gemm<2>(acc, make_rsrc(ax.w_in_x2), lane16, 2 * w, ngin, ngin, xp, XP_PIECE,
                   [&](int ks, int cb) { return (unsigned)((cb * 32 + l31) * BX_PR + (ks * 16 + half * 8) * 2); });
        const rsrc_t ro = make_rsrc(a.xin_next + (int64_t)b * DC * T);
        float bin[2][16];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) bin[i][r] = (a.b_in + 32 * (2 * w + i) + urow16(r))[4 * half];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
            if (t0 + 32 * cb + l31 < T) {
                const unsigned so = Q4 ? 16u * (unsigned)(half * T + t0 + 32 * cb + l31) : 4u * (unsigned)(4 * half * T + t0 + 32 * cb + l31);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    if (Q4) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {  // registers 4 j .. 4 j + 3: rows 32 (2 w + i) + 8 j + 4 half + 0 .. 3 = one quad
                            f32x4 q;
#pragma unroll
                            for (int e = 0; e < 4; ++e) q[e] = fmaxf(acc[i][cb][4 * j + e] * inv + bin[i][4 * j + e], 0.0f);
                            buf_store4_padded<false>(q, ro, so, (unsigned)(32 * (2 * w + i) + 8 * j) * T4);
                        }
                        continue;
                    }
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int ur = 32 * (2 * w + i) + urow16(r);
                        buf_store(fmaxf(acc[i][cb][r] * inv + bin[i][r], 0.0f), ro, so, 4u * (unsigned)ur * (unsigned)T);
                    }
                }
            }
        }
    }
}

bool boundary_fusable(const SetDiffLoopArgs &a) {
    if (const char *e = getenv("SET_AMD_FUSED_BOUNDARY"))
        if (atoi(e) == 0) return false;
    return a.T % 4 == 0 && a.M <= 96 && a.M >= 2 && ((a.M + 15) / 16 * 16 / 2) % 8 == 0;
}

// plain [256][T] rows -> channel quads: thread (utterance, quad, frame) reads its four channels (coalesced over frames), writes 16 bytes
__global__ void __launch_bounds__(256) relayout_q4_kernel(const float *src, float *dst, int T, int64_t n_quads) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;  // (b * 64 + quad) * T + t
    if (i >= n_quads) return;
    const int64_t bq = i / T;
    const int t = (int)(i - bq * T);
    const float *p = src + bq * 4 * T + t;
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = p[(int64_t)e * T];
    *reinterpret_cast<f32x4 *>(dst + 4 * i) = v;
}

int launch_relayout_q4(const float *src, float *dst, int Bg, int T, hipStream_t s) {
    const int64_t n_quads = (int64_t)Bg * (DC / 4) * T;
    SET_REQUIRE((n_quads + 255) / 256 < ((int64_t)1 << 31), "set_diffusion_loop(relayout)");
    hipLaunchKernelGGL(relayout_q4_kernel, dim3((unsigned)((n_quads + 255) / 256)), dim3(256), 0, s, src, dst, T, n_quads);
    return set_check_launch("set_diffusion_loop(relayout)");
}

int launch_boundary(const SetDiffLoopArgs &a, int Bg, const float *skip, float *x, const float *eps, int sid, uint64_t quad_offset,
                    float *xin_next, bool x2, bool q4, hipStream_t s) {
    static SetDeviceOnce lds_once;
    if (int rc = set_lds_optin(lds_once, 80 * 1024, "boundary(attr)", diffnet_boundary_kernel, diffnet_boundary_x2_kernel<false>,
                               diffnet_boundary_x2_kernel<true>))
        return rc;
    SET_REQUIRE(!q4 || x2, "set_diffusion_loop(boundary: the channel-quad layout needs the two-piece fp16 boundary)");
    BoundaryArgs g = {};
    g.skip = skip; g.x = x; g.eps = eps; g.coef4 = a.coef4 + 4 * sid;
    g.w_skip_p = a.w_skip_p; g.b_skip = a.b_skip; g.w_outp_p = a.w_outp_p; g.b_outp = a.b_outp;
    g.w_in_p = a.w_in_p; g.b_in = a.b_in; g.xin_next = xin_next;
    g.div = sqrtf((float)a.L); g.seed = a.seed; g.quad_offset = quad_offset; g.seed_delta = set_seed_delta_ptr();
    g.T = a.T; g.M = a.M; g.MP = (a.M + 15) / 16 * 16;
    if (x2) {
        BoundaryX2Args gx = {};
        gx.g = g;
        gx.w_skip_x2 = reinterpret_cast<const unsigned short *>(a.w_skip_x2);
        gx.w_outp_x2 = reinterpret_cast<const unsigned short *>(a.w_outp_x2);
        gx.w_in_x2 = reinterpret_cast<const unsigned short *>(a.w_in_x2);
        gx.err_flag = a.err_flag;
        if (q4)
            hipLaunchKernelGGL(diffnet_boundary_x2_kernel<true>, dim3((a.T + 63) / 64, Bg), dim3(256), (size_t)2 * BX_PIECE, s, gx);
        else
            hipLaunchKernelGGL(diffnet_boundary_x2_kernel<false>, dim3((a.T + 63) / 64, Bg), dim3(256), (size_t)2 * BX_PIECE, s, gx);
    } else {
        hipLaunchKernelGGL(diffnet_boundary_kernel, dim3((a.T + 63) / 64, Bg), dim3(256), (size_t)DC * BD_LD * sizeof(float), s, g);
    }
    return set_check_launch("set_diffusion_loop(boundary)");
}

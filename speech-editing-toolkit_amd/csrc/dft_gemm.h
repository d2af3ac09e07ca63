// The windowed 1024-point DFT at hop 256 followed by a row matrix, both on v_mfma_f32_32x32x2_f32 with the spectrum kept on chip: the one
// kernel body behind the log-mel front end (melspec.hip) and the STOI band envelopes (stoi.hip).  What differs between the two is a policy
// P of compile-time hooks:
//   P::MB                   32-row blocks of output rows (3: n_mels <= 96; 1: <= 32 bands)
//   P::frames(len, pad)     frames of a row of `len` samples
//   P::magnitude(re, im, a) what GEMM 2 multiplies: the magnitude sqrt(re^2 + im^2 + eps), or the power re^2 + im^2
//   P::finish(v, a)         the value stored for an output row's sum v
//   GEMM 1 (fp32 MFMA): the windowed DFT as a matrix product.  A = the table W (for each bin a row win[n] cos(2 pi f n / n_fft) and a row
//     -win[n] sin(...)), B = the frames, which are never materialised: frame t, sample n = 256 q + c is y[(t + q) hop + c], read from an LDS
//     image S[c][u] (c = sample within a hop, u = hop of the tile, row stride 67) of the padded waveform slice -- a K = 4, Cin = 256 conv view.
//     The lanes of a B fragment read consecutive u: no bank conflict (the slice as it lies in memory would put all 32 lanes on one bank).
//   magnitude in registers: the real and imaginary accumulators of a (bin, frame) pair sit in the same register of the same lane.
//   GEMM 2 (fp32 MFMA): mel[m][t] += basis[m][bin] mag[bin][t].  The magnitude tile IS the B operand: register r of lane l holds bin row
//     urow16(r) + 4 (l >> 5) of frame l & 31, which is what k-step r of a 32x32x2 MFMA wants from that lane when the filterbank image lists
//     its bins in that order.  No exchange, no LDS.
// Block = 64 frames of one row, 4 waves; wave w takes the 32-bin chunks w, w + 4, ... with its own output accumulators, which are summed
// at the end in the fixed order (w0 + w2) + (w1 + w3) through the LDS the waveform slice no longer needs.  No atomics: two runs agree bit for
// bit, and a row of a ragged batch equals the same waveform run alone (a frame's column never meets another frame's).
#pragma once
#include "common.h"

namespace {

constexpr int MEL_NFFT = 1024, MEL_HOP = 256, MEL_NBIN_ALL = MEL_NFFT / 2 + 1;
constexpr int MEL_TT = 64;                              // frames per block
constexpr int MEL_U = MEL_TT + MEL_NFFT / MEL_HOP - 1;  // hops of waveform a tile reads: 67 (odd: the staging stores are conflict-free)
constexpr int MEL_LDS = MEL_HOP * MEL_U * 4;            // 68,608 B: two blocks per CU
constexpr int MEL_KB = 8;                               // k-steps (2 samples each) per pipelined body

// where sample i of the padded waveform of a row of `len` samples lies in the row: its index, or -1 for padding zeros
__device__ __forceinline__ int padded_index(int64_t i, int len, int pad, int reflect) {
    int64_t idx = i - pad;
    if (reflect) idx = idx < 0 ? -idx : (idx >= len ? 2 * ((int64_t)len - 1) - idx : idx);
    const bool valid = idx >= 0 && idx < len && (!reflect || i < (int64_t)len + 2 * pad);
    return valid ? (int)idx : -1;
}

// The two steps of log_mel_kernel below that the spectral backward of the mel loss (mel_loss.hip) repeats on the same table image and LDS
// slice, as functions: the staged slice and GEMM 1 of one 32-bin chunk.  Same loads, same k order, same MFMAs as the kernel body: the
// spectrum the backward recomputes has the forward's bits.  log_mel_kernel keeps its own text of the two steps: routed through these
// functions hipcc schedules and allocates its body otherwise (the device assembly of all three users changes), and the shipped instances
// stay the code they were measured as.  A change to either copy belongs in both.
__device__ __forceinline__ void dft_stage_slice(float *S, const float *__restrict__ x, int len, int t0, int pad, int reflect, int clamp_input,
                                                int tid) {
    const int64_t i0 = (int64_t)t0 * MEL_HOP + tid;
    constexpr int NB = 12;
    for (int u0 = 0; u0 < MEL_U; u0 += NB) {
        int idx[NB];
        float v[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) idx[k] = u0 + k < MEL_U ? padded_index(i0 + (int64_t)(u0 + k) * MEL_HOP, len, pad, reflect) : -1;
#pragma unroll
        for (int k = 0; k < NB; ++k) v[k] = x[idx[k] < 0 ? 0 : idx[k]];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            float w = clamp_input ? fminf(fmaxf(v[k], -1.0f), 1.0f) : v[k];
            if (u0 + k < MEL_U) S[tid * MEL_U + u0 + k] = idx[k] < 0 ? 0.0f : w;
        }
    }
}

// re / im [cb] of chunk `ch`: register r of lane l = bin row urow16(r) + 4 (l >> 5) of the chunk, frame 32 cb + (l & 31) of the tile
__device__ __forceinline__ void dft_chunk_spectrum(const float *__restrict__ table, int ch, const float *S, int lane, f32x16 (&re)[2],
                                                   f32x16 (&im)[2]) {
    const int h = lane >> 5, j = lane & 31;
    const f32x4 *__restrict__ wp = reinterpret_cast<const f32x4 *>(table) + (int64_t)ch * (MEL_NFFT / 4) * 64 + lane;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int r = 0; r < 16; ++r) re[cb][r] = im[cb][r] = 0.0f;
    f32x4 A[MEL_KB / 2], An[MEL_KB / 2];
#pragma unroll
    for (int p = 0; p < MEL_KB / 2; ++p) A[p] = wp[p * 64];
    constexpr int NBODY = MEL_NFFT / 2 / MEL_KB;
    for (int body = 0; body < NBODY; ++body) {
        const int nb = body + 1 < NBODY ? body + 1 : body;  // last body: re-load itself (in bounds, unused)
#pragma unroll
        for (int p = 0; p < MEL_KB / 2; ++p) An[p] = wp[(nb * (MEL_KB / 2) + p) * 64];
        __builtin_amdgcn_sched_barrier(0);
        const int n0 = body * (2 * MEL_KB);
        const float *sp = S + ((n0 & (MEL_HOP - 1)) + h) * MEL_U + (n0 >> 8) + j;
        float B0[MEL_KB], B1[MEL_KB];
#pragma unroll
        for (int u = 0; u < MEL_KB; ++u) {
            B0[u] = sp[u * 2 * MEL_U];
            B1[u] = sp[u * 2 * MEL_U + 32];
        }
#pragma unroll
        for (int u = 0; u < MEL_KB; ++u) {
            const float ar = A[u >> 1][(u & 1) * 2], ai = A[u >> 1][(u & 1) * 2 + 1];
            re[0] = mfma32(ar, B0[u], re[0]);
            im[0] = mfma32(ai, B0[u], im[0]);
            re[1] = mfma32(ar, B1[u], re[1]);
            im[1] = mfma32(ai, B1[u], im[1]);
        }
#pragma unroll
        for (int p = 0; p < MEL_KB / 2; ++p) A[p] = An[p];
    }
}

template <class P>
__global__ void __launch_bounds__(256, 2) log_mel_kernel(SetLogMelArgs a, int nchunks) {
    extern __shared__ __attribute__((aligned(16))) float S[];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.y, t0 = blockIdx.x * MEL_TT;
    int64_t len64 = a.lengths ? a.lengths[b] : (int64_t)a.N;
    const int len = (int)(len64 < 0 ? 0 : (len64 > a.N ? a.N : len64));
    const int Tb = P::frames(len, a.pad);
    float *__restrict__ out = a.mel + (int64_t)b * a.T * a.n_mels;
    if (t0 >= Tb) {  // a tile of collater padding only (block-uniform: no barrier is skipped by part of a block)
        const int t1 = min(t0 + MEL_TT, a.T);
        for (int i = t0 * a.n_mels + tid; i < t1 * a.n_mels; i += 256) out[i] = 0.0f;
        return;
    }
    // ---- stage the slice: thread = sample within a hop (coalesced reads along the waveform, LDS stores at the odd stride)
    {
        const float *__restrict__ x = a.wav + (int64_t)b * a.wav_bs;
        const int64_t i0 = (int64_t)t0 * MEL_HOP + tid;
        if (len == 0) {  // block-uniform; an empty row still has the one frame of its padding
            for (int u = 0; u < MEL_U; ++u) S[tid * MEL_U + u] = 0.0f;
        } else {
            // batches of loads in flight: a sample that is padding reads x[0] (inside the row: len >= 1) and drops it
            constexpr int NB = 12;
            for (int u0 = 0; u0 < MEL_U; u0 += NB) {
                int idx[NB];
                float v[NB];
#pragma unroll
                for (int k = 0; k < NB; ++k) idx[k] = u0 + k < MEL_U ? padded_index(i0 + (int64_t)(u0 + k) * MEL_HOP, len, a.pad, a.reflect) : -1;
#pragma unroll
                for (int k = 0; k < NB; ++k) v[k] = x[idx[k] < 0 ? 0 : idx[k]];
#pragma unroll
                for (int k = 0; k < NB; ++k) {
                    float w = a.clamp_input ? fminf(fmaxf(v[k], -1.0f), 1.0f) : v[k];
                    if (u0 + k < MEL_U) S[tid * MEL_U + u0 + k] = idx[k] < 0 ? 0.0f : w;
                }
            }
        }
    }
    __syncthreads();

    const int h = lane >> 5, j = lane & 31;
    f32x16 mel[P::MB][2];
#pragma unroll
    for (int mb = 0; mb < P::MB; ++mb)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) mel[mb][cb][r] = 0.0f;

    for (int ch = wv; ch < nchunks; ch += 4) {
        // table image: [chunk][pair of k-steps p][lane][4] = {re, im of k-step 2p, re, im of k-step 2p + 1}: one 16-byte load per lane
        const f32x4 *__restrict__ wp = reinterpret_cast<const f32x4 *>(a.table) + (int64_t)ch * (MEL_NFFT / 4) * 64 + lane;
        f32x16 re[2], im[2];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) re[cb][r] = im[cb][r] = 0.0f;
        f32x4 A[MEL_KB / 2], An[MEL_KB / 2];
#pragma unroll
        for (int p = 0; p < MEL_KB / 2; ++p) A[p] = wp[p * 64];
        constexpr int NBODY = MEL_NFFT / 2 / MEL_KB;  // 64 bodies of 8 k-steps = 16 samples: a body never crosses a hop
        for (int body = 0; body < NBODY; ++body) {
            const int nb = body + 1 < NBODY ? body + 1 : body;  // last body: re-load itself (in bounds, unused)
#pragma unroll
            for (int p = 0; p < MEL_KB / 2; ++p) An[p] = wp[(nb * (MEL_KB / 2) + p) * 64];
            __builtin_amdgcn_sched_barrier(0);  // the next body's table loads stay in front of this body's MFMAs (a body of latency to land)
            const int n0 = body * (2 * MEL_KB);
            const float *sp = S + ((n0 & (MEL_HOP - 1)) + h) * MEL_U + (n0 >> 8) + j;
            float B0[MEL_KB], B1[MEL_KB];
#pragma unroll
            for (int u = 0; u < MEL_KB; ++u) {
                B0[u] = sp[u * 2 * MEL_U];
                B1[u] = sp[u * 2 * MEL_U + 32];
            }
#pragma unroll
            for (int u = 0; u < MEL_KB; ++u) {
                const float ar = A[u >> 1][(u & 1) * 2], ai = A[u >> 1][(u & 1) * 2 + 1];
                re[0] = mfma32(ar, B0[u], re[0]);
                im[0] = mfma32(ai, B0[u], im[0]);
                re[1] = mfma32(ar, B1[u], re[1]);
                im[1] = mfma32(ai, B1[u], im[1]);
            }
#pragma unroll
            for (int p = 0; p < MEL_KB / 2; ++p) A[p] = An[p];
        }
        // magnitude, then GEMM 2 with the magnitude registers as the B operand
        // filterbank image: [chunk][k-step r][lane][4] = basis[32 mb + (lane & 31)][bin_lo + 32 chunk + urow16(r) + 4 (lane >> 5)], mb = 0..2
        // (loaded in two halves, each pinned a phase ahead of its MFMAs: the magnitudes cover the first, the first half's MFMAs the second)
        const f32x4 *__restrict__ bp = reinterpret_cast<const f32x4 *>(a.basis) + (int64_t)ch * 16 * 64 + lane;
        f32x4 W0[8], W1[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) W0[r] = bp[r * 64];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) re[cb][r] = P::magnitude(re[cb][r], im[cb][r], a);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 8; ++r) W1[r] = bp[(8 + r) * 64];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const f32x4 w = r < 8 ? W0[r] : W1[r - 8];
#pragma unroll
            for (int mb = 0; mb < P::MB; ++mb) {
                mel[mb][0] = mfma32(w[mb], re[0][r], mel[mb][0]);
                mel[mb][1] = mfma32(w[mb], re[1][r], mel[mb][1]);
            }
        }
    }

    // ---- sum the four waves' mel accumulators: (w0 + w2) + (w1 + w3), through LDS slots of [96 registers][64 lanes]
    __syncthreads();  // every wave is done reading the waveform slice
    constexpr int SLOT = P::MB * 2 * 16 * 64;
    static_assert(2 * SLOT * 4 <= MEL_LDS, "two reduction slots fit the slice's LDS");
    auto put = [&](float *slot) {
#pragma unroll
        for (int mb = 0; mb < P::MB; ++mb)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) slot[((mb * 2 + cb) * 16 + r) * 64 + lane] = mel[mb][cb][r];
    };
    auto add = [&](const float *slot) {
#pragma unroll
        for (int mb = 0; mb < P::MB; ++mb)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int r = 0; r < 16; ++r) mel[mb][cb][r] += slot[((mb * 2 + cb) * 16 + r) * 64 + lane];
    };
    if (wv >= 2) put(S + (wv - 2) * SLOT);
    __syncthreads();
    if (wv < 2) add(S + wv * SLOT);
    __syncthreads();
    if (wv == 1) put(S);
    __syncthreads();
    if (wv != 0) return;
    add(S);

    // ---- epilogue (wave 0): log_scale * log(max(mel, floor)) in double, rounded once; frames at or beyond T_b are the pad value 0.0.
    //      Registers 4g .. 4g+3 of a lane are four consecutive mel rows of its frame: one 16-byte store when n_mels allows it.
    const bool vec = (a.n_mels & 3) == 0;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) {
        const int t = t0 + cb * 32 + j;
        if (t >= a.T) continue;
        const unsigned live = t < Tb ? 0xffffffffu : 0u;  // the log is finite (floor > 0): masked to +0.0, not a branch per element
        float *__restrict__ o = out + (int64_t)t * a.n_mels;
#pragma unroll
        for (int mb = 0; mb < P::MB; ++mb)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int m0 = mb * 32 + 8 * g + 4 * h;
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    v[e] = __builtin_bit_cast(
                        float, __builtin_bit_cast(unsigned, P::finish(mel[mb][cb][4 * g + e], a)) & live);
                if (vec) {
                    if (m0 < a.n_mels) *reinterpret_cast<f32x4 *>(o + m0) = v;
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (m0 + e < a.n_mels) o[m0 + e] = v[e];
                }
            }
    }
}

}  // namespace

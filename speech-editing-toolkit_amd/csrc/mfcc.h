// The cepstrum kernel behind set_mfcc (mcd.hip) and set_db_mfcc (wav_mcd.hip), and the clamped read of a row's length both files use.
//   out[b][t][k] = sum_n x[b][t][n] table[k][n]: a plain fp32 FMA chain in ascending n against a host-built table, table and 16 frames in
//   LDS; ~3 k MACs per frame.  What x is depends on DB:
//     DB = false   x = mel, or log10(mel) rounded once from double with take_log
//     DB = true    x = max(dB, peak[b] - top_db): librosa.power_to_db's clamp under the utterance's own peak (one fp32 subtraction)
//   Rows t >= lengths[b] are +0.0 and are never read.
#pragma once
#include "common.h"

namespace {

constexpr int MCD_K_MAX = 64, MCD_M_MAX = 96;
constexpr int MFCC_FR = 16;  // frames per block

// a row's length, read as the caller wrote it but never outside [lo, T]: the kernels stay inside their buffers whatever the device holds
__device__ __forceinline__ int row_len(const int64_t *p, int b, int lo, int T) {
    const int64_t v = p ? p[b] : (int64_t)T;
    return (int)(v < lo ? lo : (v > T ? T : v));
}

template <bool DB>
__global__ void __launch_bounds__(256) mfcc_kernel(const float *__restrict__ mel, const int64_t *__restrict__ lengths,
                                                   const float *__restrict__ table, float *__restrict__ out, int T, int M, int K, int take_log,
                                                   const float *__restrict__ peak, float top_db) {
    __shared__ float xs[MFCC_FR][MCD_M_MAX];
    __shared__ float ts[MCD_K_MAX * (MCD_M_MAX + 1)];  // row stride 97: lanes at different k, same n, on different banks
    const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * MFCC_FR;
    const int len = row_len(lengths, b, 0, T);
    const float lo = DB ? __fsub_rn(peak[b], top_db) : 0.0f;
    for (int e = tid; e < K * M; e += 256) {
        const int k = e / M;
        ts[k * (MCD_M_MAX + 1) + (e - k * M)] = table[e];
    }
    for (int e = tid; e < MFCC_FR * M; e += 256) {
        const int f = e / M, n = e - f * M, t = t0 + f;
        float v = 0.0f;
        if (t < len) {
            v = mel[((int64_t)b * T + t) * M + n];
            if (DB) v = fmaxf(v, lo);
            else if (take_log) v = (float)log10((double)v);  // rounded once
        }
        xs[f][n] = v;
    }
    __syncthreads();
    for (int e = tid; e < MFCC_FR * K; e += 256) {
        const int f = e / K, k = e - f * K, t = t0 + f;
        if (t >= T) break;
        float acc = 0.0f;
        for (int n = 0; n < M; ++n) acc = __builtin_fmaf(xs[f][n], ts[k * (MCD_M_MAX + 1) + n], acc);
        out[((int64_t)b * T + t) * K + k] = t < len ? acc : 0.0f;
    }
}

}  // namespace

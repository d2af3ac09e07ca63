// Short-time objective intelligibility on the device (eval/stoi.py `stoi`, non-extended, at its own constants: 1024-sample frames, 15
// third-octave bands, 30-frame segments, BETA = -15 dB, 40 dB dynamic range; include/set_amd.h states the arithmetic).
//   set_stoi_select   frame energies of x at hop 512 and the list of frames within 40 dB of the loudest (eval/utils.py
//                     `remove_silent_frames`): one block per row; a wave per frame, lanes over the samples, a butterfly sum; then the
//                     flags are scanned 256 frames at a time (ballot + popcount inside a wave, the four wave totals through LDS).
//   set_stoi_compact  `_overlap_and_add` of the kept windowed frames, for x and for y with x's list: one block per 512 output samples of
//                     a pair, two separately rounded products and one rounded add per sample.
//   set_stoi_bands    band envelopes: log_mel_kernel<P> of dft_gemm.h with the power in place of the magnitude, one 32-row block for the
//                     0/1 band matrix, and a square root for the log.  No padding: frame m starts at 256 m.
//   set_stoi_score    one block per pair.  The envelopes pass through LDS in tiles of 128 segments with a 29-frame halo; a thread takes the
//                     (segment, band) items tid, tid + 256, ... of each tile and evaluates each directly (three passes over its 30 frames,
//                     in double); its sum runs over the tiles in order, then a fixed LDS tree.  The partition depends on T_b only.
// No atomics anywhere: two runs agree bit for bit, and a row of a ragged batch equals the same pair run alone.
#include "dft_gemm.h"

namespace {

constexpr int STOI_FRAME = 1024, STOI_EHOP = STOI_FRAME / 2;  // energy / overlap-add frames: 1024 samples at hop 512
constexpr int STOI_SEG = 30;                                   // frames per intermediate-intelligibility segment
constexpr int STOI_TS = 128;                                   // segments per LDS tile of the score kernel
constexpr int STOI_NB_MAX = 32;                                // bands: one 32-row MFMA block
constexpr float STOI_EPS = 2.220446e-16f;
constexpr float STOI_RANGE = 0.01f;                            // -40 dB on a norm

// a row's length in samples, read as the caller wrote it but never outside [0, N]
__device__ __forceinline__ int stoi_len(const int64_t *p, int b, int N) {
    const int64_t v = p ? p[b] : (int64_t)N;
    return (int)(v < 0 ? 0 : (v > N ? N : v));
}
// frames of `frame` samples at hop `hop` that start in front of len - frame (the reference's range(0, len - frame, hop))
__device__ __forceinline__ int stoi_frames(int len, int hop) { return len > STOI_FRAME ? (len - STOI_FRAME + hop - 1) / hop : 0; }

__global__ void __launch_bounds__(256) stoi_select_kernel(const float *__restrict__ x, int64_t x_bs, const int64_t *__restrict__ lengths,
                                                          const float *__restrict__ win, float *__restrict__ nrm, int32_t *__restrict__ kept,
                                                          int32_t *__restrict__ K, int N, int Fmax) {
    __shared__ float w[STOI_FRAME];
    __shared__ float wmax[4];
    __shared__ int wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, b = blockIdx.x;
    const int F = stoi_frames(stoi_len(lengths, b, N), STOI_EHOP);
    const float *__restrict__ xb = x + (int64_t)b * x_bs;
    float *__restrict__ nb = nrm + (int64_t)b * Fmax;
    int32_t *__restrict__ kb = kept + (int64_t)b * Fmax;
    for (int n = tid; n < STOI_FRAME; n += 256) w[n] = win[n];
    __syncthreads();
    // ---- energies: lane l sums samples l, l + 64, ... in ascending order, then the butterfly 32, 16, ..., 1 (every lane ends with the sum)
    float mx = 0.0f;
    for (int f = wv; f < F; f += 4) {
        const float *__restrict__ xf = xb + (int64_t)f * STOI_EHOP;
        float acc = 0.0f;
#pragma unroll
        for (int k = 0; k < STOI_FRAME / 64; ++k) {
            const float p = __fmul_rn(w[lane + 64 * k], xf[lane + 64 * k]);
            acc = __fadd_rn(acc, __fmul_rn(p, p));
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, off));
        const float nr = __fsqrt_rn(acc);
        if (lane == 0) nb[f] = nr;
        mx = fmaxf(mx, nr);
    }
    if (lane == 0) wmax[wv] = mx;
    __syncthreads();  // (also: the norms written above are visible to the whole block)
    const float thr = __fmul_rn(STOI_RANGE, __fadd_rn(fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3])), STOI_EPS));
    // ---- selection and its scan, 256 frames at a time
    int run = 0;
    for (int base = 0; base < F; base += 256) {  // block-uniform
        const int f = base + tid;
        const bool keep = f < F && __fadd_rn(nb[f], STOI_EPS) > thr;
        const unsigned long long m = __ballot(keep);
        if (lane == 0) wtot[wv] = __popcll(m);
        __syncthreads();
        int off = run;
        for (int v = 0; v < wv; ++v) off += wtot[v];
        if (keep) kb[off + __popcll(m & ((1ull << lane) - 1ull))] = f;
        run += wtot[0] + wtot[1] + wtot[2] + wtot[3];
        __syncthreads();  // wtot is free for the next round
    }
    if (tid == 0) K[b] = run;
}

__global__ void __launch_bounds__(256) stoi_compact_kernel(const float *__restrict__ x, const float *__restrict__ y, int64_t in_bs,
                                                           const float *__restrict__ win, const int32_t *__restrict__ kept,
                                                           const int32_t *__restrict__ K, float *__restrict__ sil, int64_t sil_bs,
                                                           int64_t *__restrict__ sil_len, int B, int Fmax) {
    const int tid = threadIdx.x, j = blockIdx.x, b = blockIdx.y;
    const int Kb = min(max(K[b], 0), Fmax);
    if (j > Kb) return;  // nothing at or beyond 512 (K + 1) is written
    if (j == 0 && tid == 0) sil_len[b] = sil_len[B + b] = (int64_t)STOI_EHOP * (Kb + 1);
    const int32_t *__restrict__ kb = kept + (int64_t)b * Fmax;
    // head of kept frame j and tail of kept frame j - 1; a frame index is read clamped into [0, Fmax): 512 (Fmax - 1) + 1023 < N
    const int fa = j < Kb ? min(max(kb[j], 0), Fmax - 1) : -1;
    const int fb = j > 0 ? min(max(kb[j - 1], 0), Fmax - 1) : -1;
#pragma unroll
    for (int sig = 0; sig < 2; ++sig) {
        const float *__restrict__ s = (sig ? y : x) + (int64_t)b * in_bs;
        float *__restrict__ o = sil + ((int64_t)sig * B + b) * sil_bs + (int64_t)j * STOI_EHOP;
#pragma unroll
        for (int r = tid; r < STOI_EHOP; r += 256) {
            const float pa = fa >= 0 ? __fmul_rn(win[r], s[(int64_t)fa * STOI_EHOP + r]) : 0.0f;
            const float pb = fb >= 0 ? __fmul_rn(win[r + STOI_EHOP], s[(int64_t)fb * STOI_EHOP + STOI_EHOP + r]) : 0.0f;
            o[r] = __fadd_rn(pa, pb);  // an absent term is +0.0, as the zero padding of the reference's overlap-add
        }
    }
}

struct StoiBandPolicy {
    static constexpr int MB = 1;  // <= 32 bands
    static __device__ __forceinline__ int frames(int len, int) { return stoi_frames(len, MEL_HOP); }
    static __device__ __forceinline__ float magnitude(float re, float im, const SetLogMelArgs &) { return re * re + im * im; }
    static __device__ __forceinline__ float finish(float v, const SetLogMelArgs &) { return __fsqrt_rn(v); }
};

__global__ void __launch_bounds__(256) stoi_score_kernel(const float *__restrict__ tob, const int64_t *__restrict__ lens, float *__restrict__ d,
                                                         uint8_t *__restrict__ valid, int B, int T, int NB) {
    __shared__ float xs[(STOI_TS + STOI_SEG - 1) * STOI_NB_MAX];
    __shared__ float ys[(STOI_TS + STOI_SEG - 1) * STOI_NB_MAX];
    __shared__ double red[256];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int Tb = stoi_frames(stoi_len(lens, b, STOI_FRAME + MEL_HOP * T), MEL_HOP);  // <= T
    if (Tb < STOI_SEG) {  // block-uniform
        if (tid == 0) {
            d[b] = __builtin_nanf("");
            valid[b] = 0;
        }
        return;
    }
    const int J = Tb - (STOI_SEG - 1);
    const float *__restrict__ tx = tob + (int64_t)b * T * NB;
    const float *__restrict__ ty = tob + ((int64_t)B + b) * T * NB;
    const double clip = 1.0 + 5.623413251903491;  // 1 + 10^(-BETA / 20), BETA = -15
    double part = 0.0;
    for (int m0 = 0; m0 < J; m0 += STOI_TS) {
        const int ns = min(STOI_TS, J - m0), nf = ns + STOI_SEG - 1;
        __syncthreads();  // the tile before is done with
        for (int e = tid; e < nf * NB; e += 256) {
            xs[e] = tx[(int64_t)m0 * NB + e];
            ys[e] = ty[(int64_t)m0 * NB + e];
        }
        __syncthreads();
        for (int e = tid; e < ns * NB; e += 256) {  // item e = segment e / NB, band e % NB; its frame k is element e + k NB
            double sx = 0.0, sxx = 0.0, syy = 0.0;
            for (int k = 0; k < STOI_SEG; ++k) {
                const double xv = xs[e + k * NB], yv = ys[e + k * NB];
                sx += xv;
                sxx += xv * xv;
                syy += yv * yv;
            }
            const double ny = sqrt(syy), c = ny > 0.0 ? sqrt(sxx) / ny : 0.0;
            double sy = 0.0;
            for (int k = 0; k < STOI_SEG; ++k) sy += fmin(ys[e + k * NB] * c, xs[e + k * NB] * clip);
            const double mx = sx / STOI_SEG, my = sy / STOI_SEG;
            double dxx = 0.0, dyy = 0.0, dxy = 0.0;
            for (int k = 0; k < STOI_SEG; ++k) {
                const double dx = xs[e + k * NB] - mx, dy = fmin(ys[e + k * NB] * c, xs[e + k * NB] * clip) - my;
                dxx += dx * dx;
                dyy += dy * dy;
                dxy += dx * dy;
            }
            part += dxx > 0.0 && dyy > 0.0 ? dxy / (sqrt(dxx) * sqrt(dyy)) : 0.0;
        }
    }
    red[tid] = part;
    for (int off = 128; off > 0; off >>= 1) {
        __syncthreads();
        if (tid < off) red[tid] += red[tid + off];
    }
    if (tid == 0) {
        d[b] = (float)(red[0] / ((double)NB * (double)J));
        valid[b] = 1;
    }
}

}  // namespace

extern "C" int set_stoi_select(const float *x, int64_t x_bs, const int64_t *lengths, const float *win, float *nrm, int32_t *kept, int32_t *K,
                               int32_t B, int32_t N, int32_t n_frame, void *stream) {
    SET_REQUIRE(x && win && nrm && kept && K, "set_stoi_select");
    SET_REQUIRE(B > 0 && B <= 65535 && N > 0 && x_bs >= N && n_frame > 0, "set_stoi_select");
    if (n_frame != STOI_FRAME) return set_fail(SET_E_UNSUPPORTED, "set_stoi_select", "built for 1024-sample frames at hop 512");
    SET_REQUIRE(N > STOI_FRAME, "set_stoi_select");
    const int Fmax = (N - STOI_FRAME + STOI_EHOP - 1) / STOI_EHOP;
    hipLaunchKernelGGL(stoi_select_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x, x_bs, lengths, win, nrm, kept, K, N, Fmax);
    return set_check_launch("set_stoi_select");
}

extern "C" int set_stoi_compact(const float *x, const float *y, int64_t in_bs, const float *win, const int32_t *kept, const int32_t *K,
                                float *sil, int64_t sil_bs, int64_t *sil_len, int32_t B, int32_t N, int32_t n_frame, void *stream) {
    SET_REQUIRE(x && y && win && kept && K && sil && sil_len, "set_stoi_compact");
    SET_REQUIRE(B > 0 && B <= 65535 && N > 0 && in_bs >= N && n_frame > 0, "set_stoi_compact");
    if (n_frame != STOI_FRAME) return set_fail(SET_E_UNSUPPORTED, "set_stoi_compact", "built for 1024-sample frames at hop 512");
    SET_REQUIRE(N > STOI_FRAME, "set_stoi_compact");
    const int Fmax = (N - STOI_FRAME + STOI_EHOP - 1) / STOI_EHOP;
    SET_REQUIRE(sil_bs >= (int64_t)STOI_EHOP * (Fmax + 1), "set_stoi_compact");
    hipLaunchKernelGGL(stoi_compact_kernel, dim3(Fmax + 1, B), dim3(256), 0, (hipStream_t)stream, x, y, in_bs, win, kept, K, sil, sil_bs, sil_len,
                       B, Fmax);
    return set_check_launch("set_stoi_compact");
}

extern "C" int set_stoi_bands(const float *sil, int64_t sil_bs, const int64_t *lens, const float *table, const float *basis, float *tob,
                              int32_t R, int32_t N, int32_t T, int32_t n_fft, int32_t hop, int32_t n_bands, int32_t bin_lo, int32_t nbins,
                              void *stream) {
    SET_REQUIRE(sil && table && basis && tob, "set_stoi_bands");
    SET_REQUIRE(R > 0 && R <= 65535 && N > 0 && T > 0 && sil_bs >= N && n_fft > 0 && hop > 0 && n_bands > 0, "set_stoi_bands");
    if (n_fft != MEL_NFFT || hop != MEL_HOP || n_bands > STOI_NB_MAX)
        return set_fail(SET_E_UNSUPPORTED, "set_stoi_bands", "built for n_fft = 1024, hop = 256, <= 32 bands");
    SET_REQUIRE(bin_lo >= 0 && bin_lo % 32 == 0 && nbins > 0 && bin_lo + nbins <= MEL_NBIN_ALL, "set_stoi_bands");
    SET_REQUIRE(N > MEL_NFFT && T == (N - MEL_NFFT + MEL_HOP - 1) / MEL_HOP, "set_stoi_bands");
    SET_REQUIRE((int64_t)R * T * n_bands < (int64_t)1 << 40, "set_stoi_bands");
    SET_REQUIRE(set_aligned16(table, basis, (n_bands & 3) == 0 ? (const void *)tob : nullptr), "set_stoi_bands");
    SetLogMelArgs a = {};
    a.wav = sil, a.lengths = lens, a.table = table, a.basis = basis, a.mel = tob;
    a.wav_bs = sil_bs, a.B = R, a.N = N, a.T = T, a.n_fft = n_fft, a.hop = hop, a.n_mels = n_bands, a.bin_lo = bin_lo, a.nbins = nbins;
    static SetDeviceOnce lds_once;
    if (int rc = set_lds_optin(lds_once, MEL_LDS, "set_stoi_bands attr", log_mel_kernel<StoiBandPolicy>)) return rc;
    const dim3 grid((T + MEL_TT - 1) / MEL_TT, R);
    hipLaunchKernelGGL(log_mel_kernel<StoiBandPolicy>, grid, dim3(256), MEL_LDS, (hipStream_t)stream, a, (nbins + 31) / 32);
    return set_check_launch("set_stoi_bands");
}

extern "C" int set_stoi_score(const float *tob, const int64_t *lens, float *d, uint8_t *valid, int32_t B, int32_t T, int32_t n_bands, int32_t seg,
                              void *stream) {
    SET_REQUIRE(d && valid && (tob || T == 0), "set_stoi_score");
    SET_REQUIRE(B > 0 && T >= 0 && T < (1 << 22) && n_bands > 0 && seg > 0, "set_stoi_score");
    if (n_bands > STOI_NB_MAX || seg != STOI_SEG) return set_fail(SET_E_UNSUPPORTED, "set_stoi_score", "built for <= 32 bands, 30-frame segments");
    SET_REQUIRE((int64_t)2 * B * T * n_bands < (int64_t)1 << 40, "set_stoi_score");
    hipLaunchKernelGGL(stoi_score_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, tob, lens, d, valid, B, T, n_bands);
    return set_check_launch("set_stoi_score");
}

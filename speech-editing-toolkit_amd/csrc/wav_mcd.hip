// The wav-level mel-cepstral distortion of the reference's eval script on the device (eval/mcd.py `cal_mcd`, built there on
// librosa.feature.mfcc(htk=True, n_mfcc=34); include/set_amd.h states the arithmetic).  n_fft = 1024, hop = 256.
//   set_db_mel         wav -> 10 log10(max(1e-10, B_htk |STFT|^2)): log_mel_kernel<P> of dft_gemm.h with the power of the STOI policy for the
//                      magnitude and the floor-and-log of the log-mel policy for the finish.  Reflection padding of n_fft / 2.
//   set_db_peak        peak[b] = max of dB over the row's own frames and all bands (power_to_db's reference point for top_db).  One block
//                      per row; pad frames hold +0.0 and are not read (every dB of a quiet utterance is negative).  A maximum has no
//                      rounding: any tree gives the same bits.
//   set_db_mfcc        c[b][t][k] = sum_n table[k][n] max(dB[b][t][n], peak[b] - top_db): mfcc_kernel<true> of mfcc.h against the orthonormal
//                      DCT-II table, rows 0 .. K-1.
//   set_coef_rms_dist  `cal_mcd(use_dtw=False)` as the reference wrote it: for each coefficient k the squared difference summed over the
//                      FRAMES, then mean_k(10 / ln 10 sqrt(2 s_k)) / T.  One block per pair: thread (q, k) sums t = q, q + 4, ... in
//                      ascending order in double, the four partial sums of a k are added as (0 + 1) + (2 + 3), the K terms in ascending k.
// No atomics anywhere: two runs agree bit for bit, and a row of a ragged batch equals the same pair run alone.
#include "dft_gemm.h"
#include "mfcc.h"

namespace {

struct DbMelPolicy {
    static constexpr int MB = 3;  // 32-row blocks of mel rows: n_mels <= 96
    // reflection needs more than `pad` samples: a shorter row has no frame at all
    static __device__ __forceinline__ int frames(int len, int pad) { return len > pad ? 1 + (len + 2 * pad - MEL_NFFT) / MEL_HOP : 0; }
    static __device__ __forceinline__ float magnitude(float re, float im, const SetLogMelArgs &) { return re * re + im * im; }
    // log_scale * log(max(S, floor)) in double, rounded once
    static __device__ __forceinline__ float finish(float v, const SetLogMelArgs &a) { return (float)(a.log_scale * log((double)fmaxf(v, a.floor))); }
};

__global__ void __launch_bounds__(256) db_peak_kernel(const float *__restrict__ db, const int64_t *__restrict__ frames, float *__restrict__ peak,
                                                      int T, int M) {
    __shared__ float red[256];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int64_t n = (int64_t)row_len(frames, b, 0, T) * M;
    const float *__restrict__ p = db + (int64_t)b * T * M;
    float mx = -__builtin_inff();  // a row without frames: the maximum of nothing
    for (int64_t e = tid; e < n; e += 256) mx = fmaxf(mx, p[e]);
    red[tid] = mx;
    for (int off = 128; off > 0; off >>= 1) {
        __syncthreads();
        if (tid < off) red[tid] = fmaxf(red[tid], red[tid + off]);
    }
    if (tid == 0) peak[b] = red[0];
}

constexpr int RMS_Q = 4;  // frame slices per coefficient: 4 x 64 threads

__global__ void __launch_bounds__(256) coef_rms_dist_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                            const int64_t *__restrict__ frames_x, const int64_t *__restrict__ frames_y,
                                                            float *__restrict__ mcd, uint8_t *__restrict__ valid, int Tx, int Ty, int K) {
    __shared__ double part[RMS_Q][MCD_K_MAX];
    const int tid = threadIdx.x, k = tid & 63, q = tid >> 6, b = blockIdx.x;
    const int lx = row_len(frames_x, b, 0, Tx), ly = row_len(frames_y, b, 0, Ty);
    if (lx != ly || lx < 1) {  // block-uniform; the reference would raise on unequal frame counts
        if (tid == 0) {
            mcd[b] = __builtin_nanf("");
            valid[b] = 0;
        }
        return;
    }
    const float *__restrict__ xb = x + (int64_t)b * Tx * K;
    const float *__restrict__ yb = y + (int64_t)b * Ty * K;
    double acc = 0.0;
    if (k < K)
        for (int t = q; t < lx; t += RMS_Q) {
            const double d = (double)xb[(int64_t)t * K + k] - (double)yb[(int64_t)t * K + k];
            acc += d * d;
        }
    part[q][k] = acc;
    __syncthreads();
    if (tid < K) {
        const double s = (part[0][k] + part[1][k]) + (part[2][k] + part[3][k]);
        part[0][k] = 4.3429448190325175 * sqrt(2.0 * s);  // 10 / ln 10 as float64 gives it
    }
    __syncthreads();
    if (tid == 0) {
        double sum = 0.0;
        for (int i = 0; i < K; ++i) sum += part[0][i];
        mcd[b] = (float)(sum / (double)K / (double)lx);  // T of the reference signal (= the other's: they are equal here)
        valid[b] = 1;
    }
}

}  // namespace

extern "C" int set_db_mel(const SetLogMelArgs *args, void *stream) {
    SET_REQUIRE(args != nullptr, "set_db_mel");
    const SetLogMelArgs &a = *args;
    SET_REQUIRE(a.wav && a.table && a.basis && a.mel, "set_db_mel");
    SET_REQUIRE(a.B > 0 && a.N > 0 && a.T > 0 && a.wav_bs >= a.N && a.n_fft > 0 && a.hop > 0 && a.n_mels > 0, "set_db_mel");
    if (a.n_fft != MEL_NFFT || a.hop != MEL_HOP || a.n_mels > 32 * DbMelPolicy::MB || a.pad != MEL_NFFT / 2 || a.reflect != 1)
        return set_fail(SET_E_UNSUPPORTED, "set_db_mel", "built for n_fft = 1024, hop = 256, n_mels <= 96, reflection padding of 512");
    SET_REQUIRE(a.bin_lo >= 0 && a.bin_lo % 32 == 0 && a.nbins > 0 && a.bin_lo + a.nbins <= MEL_NBIN_ALL, "set_db_mel");
    SET_REQUIRE(a.clamp_input == 0 || a.clamp_input == 1, "set_db_mel");
    SET_REQUIRE(a.N > a.pad && a.T == 1 + a.N / MEL_HOP, "set_db_mel");
    SET_REQUIRE(a.floor > 0.0f && a.log_scale > 0.0, "set_db_mel");
    SET_REQUIRE((int64_t)a.B * a.T * a.n_mels < (int64_t)1 << 40 && a.B <= 65535, "set_db_mel");
    SET_REQUIRE(set_aligned16(a.table, a.basis, (a.n_mels & 3) == 0 ? (const void *)a.mel : nullptr), "set_db_mel");
    static SetDeviceOnce lds_once;
    if (int rc = set_lds_optin(lds_once, MEL_LDS, "set_db_mel attr", log_mel_kernel<DbMelPolicy>)) return rc;
    const dim3 grid((a.T + MEL_TT - 1) / MEL_TT, a.B);
    hipLaunchKernelGGL(log_mel_kernel<DbMelPolicy>, grid, dim3(256), MEL_LDS, (hipStream_t)stream, a, (a.nbins + 31) / 32);
    return set_check_launch("set_db_mel");
}

extern "C" int set_db_peak(const float *db, const int64_t *frames, float *peak, int32_t B, int32_t T, int32_t M, void *stream) {
    SET_REQUIRE(db && peak, "set_db_peak");
    SET_REQUIRE(B > 0 && T > 0 && M > 0 && (int64_t)B * T * M < (int64_t)1 << 40, "set_db_peak");
    hipLaunchKernelGGL(db_peak_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, db, frames, peak, T, M);
    return set_check_launch("set_db_peak");
}

extern "C" int set_db_mfcc(const float *db, const int64_t *frames, const float *peak, const float *table, float *out, int32_t B, int32_t T,
                           int32_t M, int32_t K, float top_db, void *stream) {
    SET_REQUIRE(db && peak && table && out, "set_db_mfcc");
    SET_REQUIRE(B > 0 && B <= 65535 && T > 0 && M > 0 && K > 0 && top_db >= 0.0f, "set_db_mfcc");
    if (K > MCD_K_MAX || M > MCD_M_MAX) return set_fail(SET_E_UNSUPPORTED, "set_db_mfcc", "built for n_mfcc <= 64, n_mels <= 96");
    SET_REQUIRE((int64_t)B * T * M < (int64_t)1 << 40, "set_db_mfcc");
    const dim3 grid((T + MFCC_FR - 1) / MFCC_FR, B);
    hipLaunchKernelGGL(mfcc_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, db, frames, table, out, T, M, K, 0, peak, top_db);
    return set_check_launch("set_db_mfcc");
}

extern "C" int set_coef_rms_dist(const float *x, const float *y, const int64_t *frames_x, const int64_t *frames_y, float *mcd, uint8_t *valid,
                                 int32_t B, int32_t Tx, int32_t Ty, int32_t K, void *stream) {
    SET_REQUIRE(x && y && mcd && valid, "set_coef_rms_dist");
    SET_REQUIRE(B > 0 && Tx > 0 && Ty > 0 && K > 0, "set_coef_rms_dist");
    if (K > MCD_K_MAX) return set_fail(SET_E_UNSUPPORTED, "set_coef_rms_dist", "built for K <= 64");
    SET_REQUIRE((int64_t)B * Tx * K < (int64_t)1 << 40 && (int64_t)B * Ty * K < (int64_t)1 << 40, "set_coef_rms_dist");
    hipLaunchKernelGGL(coef_rms_dist_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x, y, frames_x, frames_y, mcd, valid, Tx, Ty, K);
    return set_check_launch("set_coef_rms_dist");
}

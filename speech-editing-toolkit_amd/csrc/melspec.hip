// Log-mel front end: wav [B][N] -> mel [B][T][n_mels] in one launch (utils/audio/__init__.py:64-75 `librosa_wav2spec`, and
// modules/vocoder/hifigan/mel_utils.py:59-76 `mel_spectrogram`; the two differ in padding, input clamp, magnitude epsilon, floor and log
// base only, which are arguments here).  n_fft = 1024, hop = 256.
//   The kernel body is log_mel_kernel<P> of dft_gemm.h with the policy below.
#include "dft_gemm.h"  // log_mel_kernel<P>: the kernel body, shared with stoi.hip

namespace {

struct LogMelPolicy {
    static constexpr int MB = 3;  // 32-row blocks of mel rows: n_mels <= 96
    static __device__ __forceinline__ int frames(int len, int pad) { return len + 2 * pad >= MEL_NFFT ? 1 + (len + 2 * pad - MEL_NFFT) / MEL_HOP : 0; }
    static __device__ __forceinline__ float magnitude(float re, float im, const SetLogMelArgs &a) { return sqrtf((re * re + im * im) + a.mag_eps); }
    // log_scale * log(max(mel, floor)) in double, rounded once
    static __device__ __forceinline__ float finish(float v, const SetLogMelArgs &a) { return (float)(a.log_scale * log((double)fmaxf(v, a.floor))); }
};
constexpr int MEL_MB = LogMelPolicy::MB;

}  // namespace

extern "C" int64_t set_sizeof_log_mel_args(void) { return (int64_t)sizeof(SetLogMelArgs); }

extern "C" int64_t set_log_mel_table_size(int32_t n_fft, int32_t nbins) {
    if (n_fft <= 0 || nbins <= 0) return 0;
    return 2 * (int64_t)((nbins + 31) / 32 * 32) * n_fft;
}

extern "C" int set_log_mel(const SetLogMelArgs *args, void *stream) {
    SET_REQUIRE(args != nullptr, "set_log_mel");
    const SetLogMelArgs &a = *args;
    SET_REQUIRE(a.wav && a.table && a.basis && a.mel, "set_log_mel");
    SET_REQUIRE(a.B > 0 && a.N > 0 && a.T > 0 && a.wav_bs >= a.N && a.n_fft > 0 && a.hop > 0 && a.n_mels > 0, "set_log_mel");
    if (a.n_fft != MEL_NFFT || a.hop != MEL_HOP || a.n_mels > 32 * MEL_MB)
        return set_fail(SET_E_UNSUPPORTED, "set_log_mel", "built for n_fft = 1024, hop = 256, n_mels <= 96");
    SET_REQUIRE(a.bin_lo >= 0 && a.bin_lo % 32 == 0 && a.nbins > 0 && a.bin_lo + a.nbins <= MEL_NBIN_ALL, "set_log_mel");
    SET_REQUIRE(a.pad >= 0 && a.pad <= MEL_NFFT / 2 && (a.reflect == 0 || a.reflect == 1) && (a.clamp_input == 0 || a.clamp_input == 1),
                "set_log_mel");
    SET_REQUIRE(!a.reflect || a.N > a.pad, "set_log_mel");  // torch's reflect pad refuses pad >= length too
    SET_REQUIRE((int64_t)a.N + 2 * a.pad >= MEL_NFFT && a.T == 1 + (a.N + 2 * a.pad - MEL_NFFT) / MEL_HOP, "set_log_mel");
    SET_REQUIRE(a.mag_eps >= 0.0f && a.floor > 0.0f && a.log_scale > 0.0, "set_log_mel");
    SET_REQUIRE((int64_t)a.B * a.T * a.n_mels < (int64_t)1 << 40 && a.B <= 65535, "set_log_mel");
    SET_REQUIRE(set_aligned16(a.table, a.basis, (a.n_mels & 3) == 0 ? (const void *)a.mel : nullptr), "set_log_mel");
    static SetDeviceOnce lds_once;
    if (int rc = set_lds_optin(lds_once, MEL_LDS, "set_log_mel attr", log_mel_kernel<LogMelPolicy>)) return rc;
    const dim3 grid((a.T + MEL_TT - 1) / MEL_TT, a.B);
    hipLaunchKernelGGL(log_mel_kernel<LogMelPolicy>, grid, dim3(256), MEL_LDS, (hipStream_t)stream, a, (a.nbins + 31) / 32);
    return set_check_launch("set_log_mel");
}
